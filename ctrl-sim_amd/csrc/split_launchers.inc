// The launchers of the split-operand kernel files (gemm_bf16x6.hip, ffn_fused.hip, attention_bf16x6.hip, loss.hip), which are compiled once
// per scheme into the namespaces s1 / s0 (split.h) and called through the global names that dispatch.hip forwards to the selected scheme.
// ONE list:  SPLIT_LAUNCHER(return type, name, (typed parameters), (the same as arguments))
// Included as it is, it declares the functions in the enclosing scope: by the kernel files inside their namespace SPLIT_NS, by launchers.h
// for s1, s0 and the global names.  dispatch.hip defines the macros itself and gets the forwarding definitions.
// SPLIT_FIXED: declared alike, but the global name does not follow the selected scheme (dispatch.hip says what it does instead).
#ifndef SPLIT_LAUNCHER
#define SPLIT_LAUNCHER(RET, NAME, PARAMS, ARGS) RET NAME PARAMS;
#define SPLIT_FIXED(RET, NAME, PARAMS, ARGS) RET NAME PARAMS;
#endif
// ---- gemm_bf16x6.hip
SPLIT_LAUNCHER(int, launch_gemm_nt_bf16x6,
               (const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, const float* R, int ldr, float* C, int ldc, int M,
                int N, int K, int relu, const float* ln_gamma, const float* ln_beta, hipStream_t st),
               (A, lda, W3, n_total, n0, bias, R, ldr, C, ldc, M, N, K, relu, ln_gamma, ln_beta, st))
SPLIT_LAUNCHER(int, launch_gemm_nt_bf16x6_kv,
               (const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, const float* R, int ldr, float* C, int ldc, int M,
                int N, int K, int relu, const float* ln_gamma, const float* ln_beta, void* kv_img, int kv_L, int kv_nkt, int kv_col0, int kv_Lreg,
                int kv_rep_k0, hipStream_t st),
               (A, lda, W3, n_total, n0, bias, R, ldr, C, ldc, M, N, K, relu, ln_gamma, ln_beta, kv_img, kv_L, kv_nkt, kv_col0, kv_Lreg, kv_rep_k0,
                st))
SPLIT_LAUNCHER(int, launch_gemm_nt_bf16x6_kvc,
               (const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, const float* R, int ldr, float* C, int ldc, int M,
                int N, int K, int relu, const float* ln_gamma, const float* ln_beta, void* kv_img, int kv_col0, int kv_n, const KvClassHost* kv_cls,
                hipStream_t st),
               (A, lda, W3, n_total, n0, bias, R, ldr, C, ldc, M, N, K, relu, ln_gamma, ln_beta, kv_img, kv_col0, kv_n, kv_cls, st))
SPLIT_LAUNCHER(int, launch_inproj_rs,
               (const float* A, int lda, const void* Wblk, const float* bias, float* C, int ldc, int M, int N, void* kv_img, int kv_col0, int kv_n,
                const KvClassHost* kv_cls, hipStream_t st),
               (A, lda, Wblk, bias, C, ldc, M, N, kv_img, kv_col0, kv_n, kv_cls, st))
SPLIT_LAUNCHER(int, launch_gemm256_rows,
               (const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, float* C, int ldc, const int* c_rows, int M,
                hipStream_t st),
               (A, lda, W3, n_total, n0, bias, C, ldc, c_rows, M, st))
// ---- ffn_fused.hip
SPLIT_LAUNCHER(int, launch_ffn_fused_bf16x6,
               (const float* X, int ldx, const void* W1p, const float* b1, const void* W2p, const float* b2, const float* gamma, const float* beta,
                float* Y, int ldy, int M, int F, hipStream_t st),
               (X, ldx, W1p, b1, W2p, b2, gamma, beta, Y, ldy, M, F, st))
SPLIT_LAUNCHER(int, launch_ffn_fused_pre,
               (const float* O, int ldo, const float* R, int ldr, const void* Wop, const float* bo, const float* g0, const float* be0,
                const void* W1q, const float* b1, const void* W2p, const float* b2, const float* gamma, const float* beta, float* Y, int ldy, int M,
                int F, hipStream_t st),
               (O, ldo, R, ldr, Wop, bo, g0, be0, W1q, b1, W2p, b2, gamma, beta, Y, ldy, M, F, st))
SPLIT_LAUNCHER(int, launch_outproj_ln_q,
               (const float* O, int ldo, const float* R, int ldr, const void* Wop, const float* bo, const float* g0, const float* be0,
                const void* Wqp, const float* bq, float* X1, int ldx1, float* Q, int ldq, int M, hipStream_t st),
               (O, ldo, R, ldr, Wop, bo, g0, be0, Wqp, bq, X1, ldx1, Q, ldq, M, st))
// ---- attention_bf16x6.hip
SPLIT_LAUNCHER(int, launch_attention_bf16x6,
               (int mode, const float* Q, int ldq, long q_batch_stride, const float* K, const float* V, int ldkv, long kv_batch_stride, float* O,
                int ldo, long o_batch_stride, const int* q_pos, const unsigned char* key_pad, int B, int Lq, int Lk, int A, hipStream_t st),
               (mode, Q, ldq, q_batch_stride, K, V, ldkv, kv_batch_stride, O, ldo, o_batch_stride, q_pos, key_pad, B, Lq, Lk, A, st))
SPLIT_LAUNCHER(int, launch_attention_bf16x6_pre,
               (int mode, const float* Q, int ldq, long q_batch_stride, const void* img, int nkt, float* O, int ldo, long o_batch_stride,
                const int* q_pos, const unsigned char* key_pad, int B, int Lq, int Lk, int A, int rep_keys, int rep_mult, int rep_pos0,
                const void* mask_tbl, hipStream_t st),
               (mode, Q, ldq, q_batch_stride, img, nkt, O, ldo, o_batch_stride, q_pos, key_pad, B, Lq, Lk, A, rep_keys, rep_mult, rep_pos0, mask_tbl,
                st))
SPLIT_LAUNCHER(int, launch_attention_classes,
               (int mode, const float* Q, int ldq, const void* img, float* O, int ldo, const unsigned char* key_pad, int n, const AttnClassHost* cls,
                hipStream_t st),
               (mode, Q, ldq, img, O, ldo, key_pad, n, cls, st))
SPLIT_LAUNCHER(int, launch_attn_mask_tables, (int n, const AttnClassHost* cls, hipStream_t st), (n, cls, st))
SPLIT_FIXED(size_t, attn_mask_table_bytes, (int Lq, int nkt), (Lq, nkt))
SPLIT_LAUNCHER(int, launch_kv_split,
               (const float* K, const float* V, int ldkv, long kv_batch_stride, int B, int Lk, int nkt, void* img, hipStream_t st),
               (K, V, ldkv, kv_batch_stride, B, Lk, nkt, img, st))
SPLIT_LAUNCHER(int, launch_kv_split_rows,
               (const float* K, const float* V, int ldkv, long kv_batch_stride, const int* pos, int B, int R, int nkt, void* img, hipStream_t st),
               (K, V, ldkv, kv_batch_stride, pos, B, R, nkt, img, st))
SPLIT_LAUNCHER(int, launch_kv_split_rows_classes, (const float* K, const float* V, int ldkv, int n, const KvRowsHost* cls, void* img, hipStream_t st),
               (K, V, ldkv, n, cls, img, st))
SPLIT_LAUNCHER(int, launch_kv_zero_tail, (int B, int key0, int n, int nkt, void* img, hipStream_t st), (B, key0, n, nkt, img, st))
SPLIT_LAUNCHER(int, launch_kv_zero_tails, (int n, const KvTailHost* t, int nimg, void* const* imgs, hipStream_t st), (n, t, nimg, imgs, st))
// ---- loss.hip
SPLIT_LAUNCHER(int, launch_head_ce,
               (const float* A, int lda, const void* Wblk, const float* bias, const int* tgt, int tgt_stride, long tgt_shift, long tgt_rows, int M,
                int nsm, int bps, int valid, float* LT, int sm0, hipStream_t st),
               (A, lda, Wblk, bias, tgt, tgt_stride, tgt_shift, tgt_rows, M, nsm, bps, valid, LT, sm0, st))
#undef SPLIT_LAUNCHER
#undef SPLIT_FIXED
