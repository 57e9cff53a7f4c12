// Training (e): the backward of one whole scene-encoder layer from the rows that enter it,
//   U = LayerNorm(X0 + SelfAttn(X0; key_pad) Wo^T + bo; norm1)     (scene_attn_grad.hip's forward: one source, the key-padding mask)
//   Y = LayerNorm(U + relu(U W1^T + b1) W2^T + b2; norm2)          (ffn_grad.hip's forward)
// — torch.nn.TransformerEncoderLayer, post-LN, relu — as an op: from X0, key_pad, dY and the layer's 12 fp32 master tensors to the 12
// gradients and (optionally) dX0.  The encoder's forward keeps nothing of a layer but the rows that enter it; this op RECOMPUTES U from
// them, then runs the two backward ops from the layer's output back: ffn (U, dY -> dU), self-attention (X0, dU -> dX0).  The gradient is
// that of the layer function evaluated this way on X0 as given.
//
// THE RECOMPUTE, per chunk of whole contexts, in the attention op's own arithmetic and its own workspace carve, which its backward then
// overwrites: Q | K | V = X0 Win^T + bin, O and the statistics (launch_scene_attn_chunk_fwd: steps 1 and 2 of the op's chunk loop), then
// U = LayerNorm(X0 + O Wo^T + bo) by decoder_layer_grad.hip's dl_proj_ln_kernel (launch_proj_ln).  As in the decoder layer op, O and the
// statistics are therefore computed TWICE, once here and once inside the attention op: the double computation is the accepted price of
// calling the op unchanged — the result equals the two public ops called by hand on u_out, bit for bit.
// Workspace: U, dU [B L, 256], then the two ops' carves on top of each other (they run one after the other).  No kernel of its own, no
// atomics anywhere; every workspace element that is read has been written by this call: identical bits from run to run.
// Host code only: the kernels are the ops' (build.py: HOST_ONLY).
#include "launchers.h"
#include "../../include/ctrlsim.h"

#define EL_CHK(...) do { int _e = (__VA_ARGS__); if (_e != 0) return _e; } while (0)
static inline size_t el_up(size_t n) { return (n + 255) & ~size_t(255); }      // fg_reduce.h's fg_up: the ops' carves start on 256 bytes

bool encoder_layer_grad_dims_ok(int B, int L, int F) { return F >= 1 && scene_attn_grad_dims_ok(B, L); }

EncLayerGradWs encoder_layer_grad_carve(size_t base, int B, int L, int F) {
  EncLayerGradWs w;
  const size_t n = el_up((size_t)B * L * DM * sizeof(float));
  w.U = el_up(base); w.dU = w.U + n;
  const size_t ops = w.dU + n;
  w.f = ffn_grad_carve(ops, (long)B * L, F);
  w.s = self_attn_grad_carve(ops, B, L);
  w.bytes = w.f.bytes > w.s.bytes ? w.f.bytes : w.s.bytes;
  return w;
}

int launch_encoder_layer_grad(const float* X0, int ldx, const unsigned char* key_pad, const float* dY, int lddy, const float* const* tn, int B,
                              int L, int F, char* ws, const EncLayerGradWs& w, float* grads, float* dX0, int lddx0, float* u_out,
                              hipStream_t st) {
  if (!X0 || !dY || !tn || !ws || !grads || !encoder_layer_grad_dims_ok(B, L, F) || ldx < DM || lddy < DM || (dX0 && lddx0 < DM) ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  for (int i = 0; i < 12; ++i)
    if (!tn[i]) return CTRLSIM_EINVAL;
  const float* const* fw = tn;          // linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm2.weight, norm2.bias
  const float* const* sw = tn + 6;      // self_attn: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias; norm1.weight, norm1.bias
  const long rows = (long)B * L;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *U = f(w.U), *dU = f(w.dU);
  // ---- U: the attention sublayer's output, through the attention op's chunk buffers
  for (int c0 = 0; c0 < B; c0 += w.s.chunk_ctx) {
    const int nc = B - c0 < w.s.chunk_ctx ? B - c0 : w.s.chunk_ctx;
    const long r0 = (long)c0 * L;
    EL_CHK(launch_scene_attn_chunk_fwd(X0, ldx, key_pad, sw[0], sw[1], B, L, c0, ws, w.s, st));
    EL_CHK(launch_proj_ln(f(w.s.O), sw[2], sw[3], X0 + r0 * ldx, ldx, sw[4], sw[5], U + r0 * DM, DM, nc * L, st));
  }
  if (u_out && hipMemcpyAsync(u_out, U, (size_t)rows * DM * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return CTRLSIM_ELAUNCH;
  // ---- the two ops, from the layer's output back
  const long gF = 2L * DM * F + F + 3 * DM;
  EL_CHK(launch_ffn_block_grad(U, DM, dY, lddy, fw[0], fw[1], fw[2], fw[3], fw[4], fw[5], rows, F, ws, w.f, grads, dU, DM, st));
  return launch_scene_attn_block_grad(X0, ldx, key_pad, dU, DM, sw[0], sw[1], sw[2], sw[3], sw[4], sw[5], B, L, ws, w.s, grads + gF, dX0, lddx0,
                                      st);
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_encoder_layer_grad_workspace_bytes(int B, int L, int F) {
  if (!encoder_layer_grad_dims_ok(B, L, F)) return CTRLSIM_EINVAL;
  return (int64_t)encoder_layer_grad_carve(0, B, L, F).bytes;
}
extern "C" int ctrlsim_encoder_layer_grad(const float* X0, int ldx, const uint8_t* key_pad, const float* dY, int lddy,
                                          const float* const* tensors, int B, int L, int F, void* workspace, float* grads, float* dX0,
                                          int lddx0, float* u_out, hipStream_t stream) {
  if (!encoder_layer_grad_dims_ok(B, L, F) || !workspace) return CTRLSIM_EINVAL;
  return launch_encoder_layer_grad(X0, ldx, key_pad, dY, lddy, tensors, B, L, F, static_cast<char*>(workspace),
                                   encoder_layer_grad_carve(0, B, L, F), grads, dX0, lddx0, u_out, stream);
}
