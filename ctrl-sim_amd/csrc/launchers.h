// The internal host interface of the library: every launcher that is defined in one translation unit and called from another, and the
// structs that cross between them BY VALUE and end up as kernel arguments — each declared here and nowhere else.  Host-only; included
// by the callers (forward.hip, api.hip, dispatch.hip) and by the defining files, so that a definition that drifts from its declaration
// is an overload nobody defines (a link error), not a kernel that reads garbage.  The class tables of the multi-class launches: classes.h.
#pragma once
#include "common.h"
#include "classes.h"

// ---- embed.hip
struct EmbedTables {
  const float* act;        // [V,256]      encoder.embed_action.weight
  const float* rtg_g;      // [R,256]      E_goal @ W_rtg[:, 0:256]^T   (folded)
  const float* rtg_v;      // [R,256]
  const float* rtg_r;      // [R,256]
  const float* rtg_bias;   // [256]
  const float* tstep;      // [MAXT,256]   encoder.embed_timestep.weight
  const float* agent;      // [A,256]      encoder.embed_agent_id.weight
  const float* ln_g;       // [256]        encoder.embed_ln
  const float* ln_b;
  int rtg_linear;          // Decision Transformer: the RTGs are continuous (float bits in rtg_bin) and rtg_g/v/r are single
                           // rows: embed_rtg(cat_c Linear_c(r_c)) = r_0 g + r_1 v + r_2 r + rtg_bias (pack.py fold)
  int flags;               // ctrlsim_dims.flags (include/ctrlsim.h): bit 0 = cfg.model.no_actions — the action embeddings (with their timestep
                           // and agent-id parts) are multiplied by zero before embed_ln (modules/encoder.py:129-130): an action row is
                           // LayerNorm(0) = the norm's bias; bit 2 = encode_initial_state False — the vehicles' initial-state rows are no
                           // keys of the scene encoder / the decoder's memory (modules/encoder.py:159-166): their padding byte is always 1
};
int launch_assemble_rows(int B, int Rn, int A, int tt_first, int Tn, const int* pos_new, const float* S2, const float* Gp, const float* exist,
                         const int* act_tok, const int* rtg_bin, const int* tstep, EmbedTables tb, float* Xn, hipStream_t st);
int launch_assemble_tokens(int B, int Tq, int A, int Areg, const float* S2, const float* Gp, const float* exist, const int* act_tok,
                           const int* rtg_bin, const int* tstep, EmbedTables tb, float* X, float* src, int M, int P, unsigned char* src_pad,
                           hipStream_t st);
int launch_assemble_tokens_classes(int n, const int* B, const int* A, const int* Areg, const int* M, const long* xrow, const long* srow,
                                   const long* grow, int Tq, const float* S2, const float* Gp, const float* exist, const int* act_tok,
                                   const int* rtg_bin, const int* tstep, EmbedTables tb, float* X, float* src, int P, unsigned char* src_pad,
                                   hipStream_t st);
int launch_assemble_rtg_rows(int B, int Ar, int A, int Tq, int ti, int t, int N, int Tmax, const int* ctx_scn, const int* slot_gid,
                             const int* hist_rtg, const float* exist, const int* tstep, EmbedTables tb, const int* zr, float* Xr, hipStream_t st);

// ---- map_encoder.hip
struct MapPoolWeights {
  const float* Wc2;     // [128,4,2] the same with the channels of a pair interleaved per component (packed kernel: scalar register pairs)
  const float* Wc;      // [256,4]  g_c * (W1[c,:] - column mean, b1[c] - mean(b1)): LN(W1 p + b1)_c = Wc[c] . (x,y,e,1) * rstd + ln_b[c]
  const float* G;       // [10]     upper triangle of sum_c wt_c wt_c^T / 256 (wt = Wc without the gain): var = (x,y,e,1)^T G (x,y,e,1)
  const float* ln_b;    // [256]
  const float* U;       // [256,8]
  const float* cb;      // [8]
  const float* Mt;      // [256(c),256(j)]
  const float* mb;      // [256]
  int force_pad;        // 1: cfg.model.use_map = False (ctrlsim_dims.flags bit 1) — every polyline row is key-padded: the scene encoder and the
                        // decoder's memory then hold the vehicles' initial-state rows only, as modules/encoder.py:168-170 builds them
};
int launch_map_pool(int B, int P, int NP, int M, const float* road_pts, MapPoolWeights w, float* attn_pre, unsigned char* src_pad, hipStream_t st);
int launch_map_pool_classes(int n, const int* B, const int* M, const long* pad0, int P, int NP, const float* road_pts, MapPoolWeights w,
                            float* attn_pre, unsigned char* src_pad, hipStream_t st);

// ---- context.hip
struct CtxOut {
  float* st12;            // [B, Tq, A, 12]  x,y,vx,vy,yaw,len,wid + 5 type one-hot (-1 padded slots)
  float* exist;           // [B, Tq, A]
  float* goal5;           // [B, A, 5]
  int* act_tok;           // [B, Tq, A]
  int* rtg_bin;           // [B, Tq, A, 3]
  int* tstep;             // [B, Tq]
  int* slot_gid;          // [B, A]   global vehicle index per slot, -1 = padded
  float* road_pts;        // [B, P, NP, 3]
  float* road_types;      // [B, P, 8]
};
int launch_group_build(int S, int N, int A, int T, int t, int Tmax1, double dist_thresh, const float* hist_states, const int* eval_order,
                       int has_roads, unsigned long long* persist, int* n_groups, int* grp_focal, unsigned long long* grp_ids,
                       unsigned long long* grp_members, int* own_g, int* mem_g, unsigned char* tilted, hipStream_t st);
int launch_ctx_index(int s0, int s1, int N, const int* n_groups, const int* grp_focal, const unsigned long long* grp_ids, const int* own_g,
                     const int* mem_g, int* ctx_scn, int* ctx_grp, int* own_ctx, int* own_slot, int* mem_ctx, int* mem_slot, int* ctx_base,
                     hipStream_t st);
int launch_ctx_index_classes(int s0, int s1, int N, int A, const int* n_groups, const unsigned long long* grp_ids, const int* own_g, const int* mem_g,
                             int nb, const int* sizes, int* ctx_scn, int* ctx_grp, int* ctx_row0, int* ctx_of_group, int* own_ctx, int* own_slot,
                             int* mem_ctx, int* mem_slot, hipStream_t st);
int launch_groups_changed(int S, int N, const int* n_groups, const int* grp_focal, const unsigned long long* grp_ids, const int* ref_n,
                          const int* ref_focal, const unsigned long long* ref_ids, int* flag, hipStream_t st);
int launch_group_size_hist(int S, int N, const int* n_groups, const unsigned long long* grp_ids, int nb, const int* sizes, int* hist, hipStream_t st);
int launch_build_context(int B, int N, int A, int T, int t, int Tq, int tt_first, int Tmax1, int Tmax, int P_all, int P, int NP, const int* ctx_scn,
                         const int* ctx_grp, const int* grp_focal, const unsigned long long* grp_ids, const float* hist_states, const int* hist_tok,
                         const int* hist_rtg, const double* goals, const float* types, const float* roads, const float* rtypes, const int* zero4,
                         CtxOut o, hipStream_t st);
int launch_build_context_classes(int n, const int* Bk, const int* Ak, const CtxOut* ok, int N, int T, int t, int Tq, int tt_first, int Tmax1,
                                 int Tmax, int P_all, int P, int NP, const int* ctx_scn, const int* ctx_grp, const int* grp_focal,
                                 const unsigned long long* grp_ids, const float* hist_states, const int* hist_tok, const int* hist_rtg,
                                 const double* goals, const float* types, const float* roads, const float* rtypes, const int* zero4, hipStream_t st);

// ---- window.hip: open-loop training windows cut from a device-resident dataset (the ABI entry ctrlsim_window_build lives there too)
struct ctrlsim_window_cfg;          // include/ctrlsim.h
int launch_window_build(int B, int S, int N, int Td, int T, int A, int Pmax, int P, int NP, const double* ag_data, const double* actions,
                        const double* rtgs, const double* goals5, const double* types, const double* road_points,
                        const double* road_types, const int* n_polys, const int* win_scn, const int* win_t0, const int* win_agent,
                        const ctrlsim_window_cfg& cfg, CtxOut o, unsigned char* moving, int* status, hipStream_t st);

// ---- gemm.hip, attention.hip: the f32-input MFMA family and the row-wise satellites
int launch_gemm_nt(const float* A, int lda, const float* W, int ldw, const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N,
                   int K, int relu, hipStream_t st);
int launch_layernorm256(const float* X, int ldx, const float* Radd, int ldr, const float* gamma, const float* beta, float* Y, int ldy, int rows,
                        int relu, hipStream_t st);
int launch_in_mlp(const float* X, int ldx, int kin, const float* W, const float* bias, const float* gamma, const float* beta, float* Y, int ldy,
                  int rows, hipStream_t st);
int launch_row_copy(const float* src, int lds_, float* dst, int ldd, const int* index, int rows, int width, int scatter, hipStream_t st);
int launch_attention(int mode, const float* Q, int ldq, long q_batch_stride, const float* K, const float* V, int ldkv, long kv_batch_stride, float* O,
                     int ldo, long o_batch_stride, const int* q_pos, const unsigned char* key_pad, int B, int Lq, int Lk, int A, hipStream_t st);

// ---- loss.hip (outside the scheme namespace: compiled in the two-plane build only)
int launch_row_lse(const float* L, long ld, int n, int estride, int nsm, const int* tgt, int tgt_stride, long tgt_shift, long tgt_rows, long row0,
                   int M, float* LT, int sm0, hipStream_t st);
int launch_loss_reduce(const float* LT, const float* exist, const unsigned char* moving, const float* st12, const float* fut, float* row_nll,
                       double* per_ctx, double* sums, int B, int Tq, int A, int nfut, int has_rtg, int shift, int supervise_moving, int local_frame,
                       hipStream_t st);

// ---- head_grad.hip: the loss gradient through the MLP heads (f32-input MFMA from the fp32 master weights: independent of the split)
struct HeadGradHead {
  const float *w0, *b0, *g, *be, *w3, *b3;   // mlp.0 weight / bias, mlp.1 (LayerNorm) weight / bias, mlp.3 weight / bias
  int n, nsm;                                // nsm interleaved softmaxes of n classes (future states: n = 2 T outputs, nsm = 1)
  int k;                                     // token type the head reads: row 3 i + k of X
  int kind;                                  // 0 action (coef, Trajeglish shift), 1 returns, 2 future states
  int sm0;                                   // first softmax slot in LT / first term in sums
  const int* tgt;                            // [rows, nsm] target classes (kinds 0, 1)
  long goff;                                 // float offset of the head's six tensors in `grads`
};
struct HeadGradWs { size_t Z, H, dH, G, slab, part, bytes; int chunk_rows; int ldg; };
HeadGradWs head_grad_carve(size_t base, long rows, int nmax);
struct HeadGradArgs {
  const float* X; int B, Tq, A, nfut, nheads; HeadGradHead h[3];
  const float *exist, *st12; const unsigned char* moving; long shift; int supervise_moving, local_frame; float action_coef;
  const double* sums; float *grads, *dX;
  float *Z, *H, *dH, *G, *slab, *part; int chunk_rows, ldg;
};
int launch_head_grads(const HeadGradArgs& a, hipStream_t st);

// ---- ffn_grad.hip: the backward of a post-LN feed-forward block (f32-input MFMA from the fp32 master weights)
struct FfnGradWs { size_t H, S, dS, slab, part_ln, part_cs, bytes; int chunk_rows, ldh; long nln, ncs; };
FfnGradWs ffn_grad_carve(size_t base, long rows, int F);
int launch_ffn_block_grad(const float* U, int ldu, const float* dY, int lddy, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* gamma, const float* beta, long rows, int F, char* ws, const FfnGradWs& w,
                          float* grads, float* dU, int lddu, hipStream_t st);

// ---- attn_grad.hip: the backward of a post-LN attention sublayer with a key-padding mask (f32-input MFMA from the fp32 master weights)
struct AttnGradWs { size_t KV, dKV, Q, O, S, dS, dQ, stat, slab, part_ln, part_cq, part_ck, bytes; int chunk_ctx; long nln, ncq, nck; };
AttnGradWs attn_grad_carve(size_t base, int B, int Lq, int Lk);
int launch_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* dY, int lddy,
                           const float* Win, const float* bin, const float* Wo, const float* bo, const float* gamma, const float* beta,
                           int B, int Lq, int Lk, char* ws, const AttnGradWs& w, float* grads, float* dX, int lddx, float* dMem, int lddm,
                           int accumulate_dmem, hipStream_t st);     // accumulate_dmem: dMem += this call's, instead of =
bool attn_grad_dims_ok(int B, int Lq, int Lk);
// steps 1 and 2 of the chunk of contexts from c0 on, into the op's chunk buffers (K | V of all contexts before the first chunk's)
int launch_attn_chunk_fwd(const float* X, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* Win, const float* bin,
                          int B, int Lq, int Lk, int c0, char* ws, const AttnGradWs& w, hipStream_t st);

// ---- self_attn_grad.hip: the backward of a decoder layer's self-attention sublayer under the multi-agent causal mask (contexts of 3 T A rows)
struct SelfAttnGradWs { size_t QKV, dQKV, O, S, dS, stat, slab, part_ln, part_cs, bytes; int chunk_ctx; long nln, ncs; };
SelfAttnGradWs self_attn_grad_carve(size_t base, int B, int L);
int launch_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* Win, const float* bin, const float* Wo,
                                const float* bo, const float* gamma, const float* beta, int B, int T, int A, int mask_mode, char* ws,
                                const SelfAttnGradWs& w, float* grads, float* dX, int lddx, hipStream_t st);
bool self_attn_grad_dims_ok(int B, int T, int A);
int launch_self_attn_chunk_fwd(const float* X, int ldx, const float* Win, const float* bin, int B, int L, int A, int mask_mode, int c0, char* ws,
                               const SelfAttnGradWs& w, hipStream_t st);     // steps 1 and 2 of the chunk of contexts from c0 on

// ---- decoder_layer_grad.hip: a whole decoder layer's backward from the rows that enter it (X1 and U recomputed, then the three ops above)
struct DecLayerGradWs { size_t X1, U, dU, dX1, bytes; FfnGradWs f; AttnGradWs a; SelfAttnGradWs s; };
bool decoder_layer_grad_dims_ok(int B, int T, int A, int Lk, int F);
DecLayerGradWs decoder_layer_grad_carve(size_t base, int B, int T, int A, int Lk, int F);
int launch_decoder_layer_grad(const float* X0, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* dY, int lddy,
                              const float* const* tensors, int B, int T, int A, int Lk, int F, int mask_mode, char* ws,
                              const DecLayerGradWs& w, float* grads, float* dX0, int lddx0, float* dMem, int lddm, int accumulate_dmem,
                              float* x1_out, float* u_out, hipStream_t st);
// Y = LayerNorm(R + O Wo^T + bo; gamma, beta) for `rows` rows (dl_proj_ln_kernel): O [rows, 256] dense, R / Y with leading dimensions
int launch_proj_ln(const float* O, const float* Wo, const float* bo, const float* R, long ldr, const float* gamma, const float* beta, float* Y,
                   long ldy, int rows, hipStream_t st);

// ---- scene_attn_grad.hip: the backward of a scene-encoder layer's self-attention sublayer — one source, key-padding mask; the
// workspace is self_attn_grad.hip's carve (self_attn_grad_carve(base, B, L))
bool scene_attn_grad_dims_ok(int B, int L);
int launch_scene_attn_block_grad(const float* X, int ldx, const unsigned char* key_pad, const float* dY, int lddy, const float* Win,
                                 const float* bin, const float* Wo, const float* bo, const float* gamma, const float* beta, int B, int L,
                                 char* ws, const SelfAttnGradWs& w, float* grads, float* dX, int lddx, hipStream_t st);
int launch_scene_attn_chunk_fwd(const float* X, int ldx, const unsigned char* key_pad, const float* Win, const float* bin, int B, int L, int c0,
                                char* ws, const SelfAttnGradWs& w, hipStream_t st);     // steps 1 and 2 of the chunk of contexts from c0 on

// ---- encoder_layer_grad.hip: a whole scene-encoder layer's backward from the rows that enter it (U recomputed, then the two ops)
struct EncLayerGradWs { size_t U, dU, bytes; FfnGradWs f; SelfAttnGradWs s; };
bool encoder_layer_grad_dims_ok(int B, int L, int F);
EncLayerGradWs encoder_layer_grad_carve(size_t base, int B, int L, int F);
int launch_encoder_layer_grad(const float* X0, int ldx, const unsigned char* key_pad, const float* dY, int lddy, const float* const* tensors,
                              int B, int L, int F, char* ws, const EncLayerGradWs& w, float* grads, float* dX0, int lddx0, float* u_out,
                              hipStream_t st);

// ---- sim.hip
int launch_sim_init(int S, int N, int E, const float* init_pose, const float* size, const float* edges, const unsigned char* exists, float* phys,
                    float* hist_states, unsigned char* coll, int Tmax1, float* contact_state, hipStream_t st);
int launch_sim_set_position(int S, int N, const float* xy, float* phys, hipStream_t st);
int launch_sim_step(int S, int N, int E, const int* act_tok, const double* act_f64, const double* disc6, const float* size, const float* edges,
                    const unsigned char* exists, float* phys, float* hist_states, unsigned char* coll, double* applied, int t, int Tmax1, float dt,
                    int kinematic, float* contact_state, const float* expert, hipStream_t st);

// ---- replay.hip
int launch_replay_latch(int S, int N, int t, int T1, const double* log, const float* phys, double* exist_hist, float* hist_states,
                        float* speed_hist, hipStream_t st);
int launch_replay_actions(int S, int N, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                          const unsigned char* controlled, const double* exist_hist, const float* hist_states, const float* phys,
                          const int* act_now, const double* disc6, double* act_f64, unsigned char* exists, int* hist_tok,
                          hipStream_t st);
int launch_replay_latch_views(int S, int N, int R, int t, int T1, const double* log, const float* phys, double* exist_hist,
                              float* hist_states, float* speed_hist, float* view_states, hipStream_t st);
int launch_replay_actions_views(int S, int N, int R, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                                const int* role, const double* exist_hist, const float* hist_states, const float* phys,
                                const int* act_now, const double* disc6, double* act_f64, unsigned char* exists, int* hist_tok,
                                int* view_tok, hipStream_t st);

// ---- sample.hip
int launch_sample_rtg(const float* rtg_logits, int A, int R, const int* own_ctx, const int* own_slot, const int* ctx_row0,
                      const unsigned char* tilted, const double* tilt3, const double* tilt_scn, const float* noise, uint64_t seed,
                      const int64_t* scenario_id, int t, int* hist_rtg, int S, int N, int Tmax, hipStream_t st);
int launch_sample_action(const float* act_logits, int A, int V, const int* mem_ctx, const int* mem_slot, const int* ctx_row0, float temperature,
                         double top_p, const float* noise, uint64_t seed, const int64_t* scenario_id, int t, int* hist_tok, int* act_now, int S,
                         int N, int Tmax, int zero_token, hipStream_t st);

// ---- the split-operand launchers (split_launchers.inc): each scheme's build, and the global names that dispatch.hip forwards to one of them
namespace s1 {
#include "split_launchers.inc"
}
namespace s0 {
#include "split_launchers.inc"
}
#include "split_launchers.inc"
