// Training, first stage: the gradient of the reference's training loss (models/ctrl_sim.py:48-214, final_loss = loss_action_coef *
// loss_actions + loss_rtg_goal + loss_rtg_veh + loss_rtg_road + loss_state) through the three MLP heads (modules/decoder.py:23-35,
// utils/layers.py:6-19: Z = X_k W0^T + b0, H = relu(LayerNorm(Z)), Y = H W3^T + b3) down to the decoder's output rows.  The dual of
// loss.hip: per head the logits are recomputed a bounded chunk of rows at a time, turned in place into G = dLoss/dY (the softmax
// normalised from the recomputed row itself: hg_g_ce_kernel says why), and leave as
//   dH = G W3,  dW3 = G^T H,  db3 = sum_rows G;   ReLU + LayerNorm backward (mean / rstd recomputed from Z): dgamma, dbeta, dZ;
//   dW0 = dZ^T X_k,  db0 = sum_rows dZ,  dX_k = dZ W0.
//
// ARITHMETIC: every product runs on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 operands, fp32 accumulation) from the fp32
// master weights — the same under either operand split of the forward, no packed image is read.  A gradient passes through up to three
// chained products; with fp32 operands the only error is the accumulation order, which is the reference's own error class.
//
// LOOP ORDER AND SLABS (no float atomics anywhere: identical bits from run to run).  Two sums cross workgroups:
//   * dH = G W3 sums over the classes.  A workgroup owns a 64 x 64 tile of dH and walks ALL classes of its rows itself: no partials.
//   * dW3 = G^T H (and dW0 = dZ^T X) sums over the rows.  The rows are cut into blocks of HG_KS = 1024; block z writes its own partial
//     slab [n, 256], and a second kernel adds the slabs element by element in slab order, in float64.
//   At B = 64 full-size contexts (49152 rows) that is 48 slabs of [1050, 256] fp32 per head: 52 MB written and read once, against
//   192 slabs (206 MB) with the 256-row blocks of the loss kernel, and against ~33 [rows, 256] slabs (1.6 GB) had dH been the operand
//   left in pieces (column-block-stationary).  The G chunk itself (<= 8192 rows x 1052 floats, 34 MB) stays L2 / MALL resident
//   between its three readers.  Column sums (db3, db0, dgamma, dbeta) follow the same two-stage pattern with smaller row blocks.
#include "hg_gemm.h"

#define HG_KS 1024               // rows per partial slab of a product that sums over rows
#define HG_CS_ROWS 128           // rows per partial of a column sum
#define HG_LN_ROWS 64            // rows per workgroup of the LayerNorm backward

namespace {

// (the tile product hg_gemm and the LayerNorm row hg_ln_row: hg_gemm.h.  The forward and the backward kernel below share hg_ln_row, so
// the backward's ReLU mask is the forward's)
__global__ __launch_bounds__(256) void hg_ln_fwd_kernel(const float* __restrict__ Z, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ H, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f32x4 zq = *reinterpret_cast<const f32x4*>(Z + row * DM + 4 * lane);
  const f32x4 gq = *reinterpret_cast<const f32x4*>(gamma + 4 * lane), bq = *reinterpret_cast<const f32x4*>(beta + 4 * lane);
  const float x[4] = {zq[0], zq[1], zq[2], zq[3]};
  float xh[4], rstd;
  hg_ln_row(x, xh, rstd);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fmaxf(xh[i] * gq[i] + bq[i], 0.f);
  *reinterpret_cast<f32x4*>(H + row * DM + 4 * lane) = o;
}

// dH -> dZ in place; part[block][3][256] = this block's sums over its rows of (dy xhat, dy, dZ): dgamma, dbeta, db0
__global__ __launch_bounds__(256) void hg_ln_bwd_kernel(const float* __restrict__ Z, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ dH, long rows,
                                                        float* __restrict__ part) {
  __shared__ float red[4][3][DM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const f32x4 gq = *reinterpret_cast<const f32x4*>(gamma + 4 * lane), bq = *reinterpret_cast<const f32x4*>(beta + 4 * lane);
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, sz[4] = {0.f, 0.f, 0.f, 0.f};
  const long r0 = (long)blockIdx.x * HG_LN_ROWS + wave * (HG_LN_ROWS / 4);
  for (int j = 0; j < HG_LN_ROWS / 4; ++j) {
    const long row = r0 + j;
    if (row >= rows) break;                            // (wave-uniform)
    const f32x4 zq = *reinterpret_cast<const f32x4*>(Z + row * DM + 4 * lane);
    const f32x4 dq = *reinterpret_cast<const f32x4*>(dH + row * DM + 4 * lane);
    const float x[4] = {zq[0], zq[1], zq[2], zq[3]};
    float xh[4], rstd, dxh[4], s1 = 0.f, s2 = 0.f;
    hg_ln_row(x, xh, rstd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = xh[i] * gq[i] + bq[i];
      const float dy = y > 0.f ? dq[i] : 0.f;
      sg[i] += dy * xh[i];
      sb[i] += dy;
      dxh[i] = dy * gq[i];
      s1 += dxh[i];
      s2 += dxh[i] * xh[i];
    }
    const float c1 = wave_sum(s1) * (1.0f / DM), c2 = wave_sum(s2) * (1.0f / DM);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = rstd * (dxh[i] - c1 - xh[i] * c2);
      sz[i] += o[i];
    }
    *reinterpret_cast<f32x4*>(dH + row * DM + 4 * lane) = o;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[wave][0][4 * lane + i] = sg[i];
    red[wave][1][4 * lane + i] = sb[i];
    red[wave][2][4 * lane + i] = sz[i];
  }
  __syncthreads();
  const int c = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    part[((long)blockIdx.x * 3 + q) * DM + c] = (red[0][q][c] + red[1][q][c]) + (red[2][q][c] + red[3][q][c]);
}

int hg_gemm(int a_kc, int b_kc, const HgGemm& g, hipStream_t st) {
  if (a_kc && b_kc) return hg_gemm_t<true, true, HG_EPI_PLAIN>(g, st);
  if (a_kc) return hg_gemm_t<true, false, HG_EPI_PLAIN>(g, st);
  if (!b_kc) return hg_gemm_t<false, false, HG_EPI_PLAIN>(g, st);
  return CTRLSIM_EINVAL;
}

// ---- logits -> G = dLoss / dY, in place, one wave per row of the chunk.  Softmax s of a row is the elements e nsm + s (action head:
// nsm = 1; return head: bin-major, component-minor).  G = (softmax(Y) - [e == target]) coef mask / count, mask and count those of
// launch_loss_reduce (loss.hip), count = sums[2 term + 1] on the device.  Columns [n nsm, ld) <- 0.
// The softmax is normalised HERE, from the row's own maximum and exp sum, as exp(y - max) / sum — not as exp(y - lse) with the
// log-sum-exp the loss pass left in LT.  Measured on the first device run (profiles/head_grad_parity.md): with LT's lse every tensor
// sat 5 - 16 x above the reference's own float32 error.  Two causes, both in the lse: it is ONE fp32 number of the logits' magnitude
// (|lse| ~ 30 with trained-like heads: half an ulp is 1e-6, a relative error of 1e-6 in every probability of the row, where
// log_softmax only rounds y - max, which is ~ 0 for the classes that carry the probability), and it came from ANOTHER evaluation of
// the logits (the forward's split-operand product), so the row's probabilities no longer summed to 1 to rounding.
struct HgRowCtx {
  const float* exist; const unsigned char* moving; const double* sums; int Tq, A, supervise_moving; long rows;
};
__global__ __launch_bounds__(256) void hg_g_ce_kernel(float* __restrict__ G, long ld, int n, int nsm, long row0, int nr, int sm0,
                                                      const int* __restrict__ tgt, long shift, int action, float coef, HgRowCtx c) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nr) return;                                 // (wave-uniform: a wave owns a row)
  const long ig = row0 + i;
  const int TA = c.Tq * c.A;
  const int rem = (int)(ig % TA), tt = rem / c.A, ag = rem - tt * c.A;
  const long b = ig / TA;
  const double mov = (c.supervise_moving && c.moving) ? (double)(c.moving[b * c.A + ag] != 0) : 1.0;
  double m = (double)c.exist[ig] * mov;
  if (action && shift) m = tt + 1 < c.Tq ? (double)c.exist[ig + c.A] * mov : 0.0;
  float* p = G + i * ld;
  const int width = n * nsm;
  float mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sm[3] = {0.f, 0.f, 0.f};
  for (int idx = lane; idx < width; idx += 64) {
    const int s = idx % nsm;
    const float y = p[idx];
    if (s == 0) mx[0] = fmaxf(mx[0], y); else if (s == 1) mx[1] = fmaxf(mx[1], y); else mx[2] = fmaxf(mx[2], y);
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) mx[s] = wave_max(mx[s]);
  for (int idx = lane; idx < width; idx += 64) {
    const int s = idx % nsm;
    const float y = p[idx];
    if (s == 0) sm[0] += expf(y - mx[0]); else if (s == 1) sm[1] += expf(y - mx[1]); else sm[2] += expf(y - mx[2]);
  }
  float sc[3], inv[3];
  int tg[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    inv[s] = 1.0f / wave_sum(sm[s]);
    sc[s] = 0.f; tg[s] = -1;
    if (s < nsm) {
      sc[s] = (float)((double)coef * m / c.sums[2 * (sm0 + s) + 1]);
      tg[s] = ig + shift < c.rows ? tgt[(ig + shift) * nsm + s] : -1;
    }
  }
  for (int idx = lane; idx < (int)ld; idx += 64) {
    if (idx >= width) { p[idx] = 0.f; continue; }
    const int e = idx / nsm, s = idx - e * nsm;
    const float scale = s == 0 ? sc[0] : s == 1 ? sc[1] : sc[2];
    const float mxs = s == 0 ? mx[0] : s == 1 ? mx[1] : mx[2];
    const float is = s == 0 ? inv[0] : s == 1 ? inv[1] : inv[2];
    const int t = s == 0 ? tg[0] : s == 1 ? tg[1] : tg[2];
    p[idx] = (expf(p[idx] - mxs) * is - (e == t ? 1.f : 0.f)) * scale;
  }
}
// future-state head: G = 2 (pred - target) mask_{tt + 1 + j} / (200 count); targets and masks of loss_ctx_kernel (world / local frame)
__global__ __launch_bounds__(256) void hg_g_state_kernel(float* __restrict__ G, long ld, int nfut, long row0, int nr,
                                                         const float* __restrict__ st12, int local_frame, HgRowCtx c) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)nr * nfut) return;
  const long i = id / nfut;
  const int j = (int)(id - i * nfut);
  const long ig = row0 + i;
  const int TA = c.Tq * c.A;
  const int rem = (int)(ig % TA), tt = rem / c.A, ag = rem - tt * c.A;
  const long b = ig / TA;
  const double mov = (c.supervise_moving && c.moving) ? (double)(c.moving[b * c.A + ag] != 0) : 1.0;
  const double mstate = local_frame ? 1.0 : mov;
  double m = 0.0, tx = 0.0, ty = 0.0;
  if (tt + 1 + j < c.Tq) {
    const long i2 = ig + (long)(1 + j) * c.A;
    m = (double)c.exist[i2] * mstate;
    if (m != 0.0) {
      tx = st12[i2 * 12]; ty = st12[i2 * 12 + 1];
      if (local_frame) {
        const double ox = st12[ig * 12], oy = st12[ig * 12 + 1], yaw = st12[ig * 12 + 4];
        const double cy = cos(-yaw), sy = sin(-yaw), dx = tx - ox, dy = ty - oy;
        tx = cy * dx - sy * dy; ty = sy * dx + cy * dy;
      }
    }
  }
  const double den = 200.0 * c.sums[9];
  float* p = G + i * ld + 2 * j;
  p[0] = (float)(2.0 * ((double)p[0] - tx) * m / den);
  p[1] = (float)(2.0 * ((double)p[1] - ty) * m / den);
}

// ---- column sums in two stages: part[block][n] over HG_CS_ROWS rows each, then the partials in block order, float64
__global__ __launch_bounds__(256) void hg_colsum_kernel(const float* __restrict__ P, long ld, int rows, int n, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int r0 = blockIdx.y * HG_CS_ROWS, r1 = min(rows, r0 + HG_CS_ROWS);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += P[(long)r * ld + c];
  part[(long)blockIdx.y * n + c] = s;
}
__global__ __launch_bounds__(256) void hg_reduce_kernel(const float* __restrict__ part, int nslab, long stride, long n, float* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s += (double)part[(long)k * stride + e];
  out[e] = (float)s;
}
int hg_reduce(const float* part, int nslab, long stride, long n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, nslab, stride, n, out);
  return ctrlsim_launch_status();
}

inline size_t hg_up(size_t n) { return (n + 255) & ~size_t(255); }

#define HG_CHK(x) do { int _e = (x); if (_e != 0) return _e; } while (0)

}  // namespace

// Workspace behind `base`: Z, H, dH [rows, 256], the G chunk [chunk_rows, ldg], the product slabs and the column-sum partials.
HeadGradWs head_grad_carve(size_t base, long rows, int nmax) {
  HeadGradWs w;
  size_t off = hg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += hg_up(n); return o; };
  w.chunk_rows = rows < 8192 ? (int)rows : 8192;
  w.ldg = (nmax + 3) & ~3;
  const long nchunks = (rows + w.chunk_rows - 1) / w.chunk_rows;
  const long nslab = (rows + HG_KS - 1) / HG_KS + nchunks;
  const long wide = w.ldg > DM ? w.ldg : DM;
  const long ncs = (rows + HG_CS_ROWS - 1) / HG_CS_ROWS + nchunks, nln = (rows + HG_LN_ROWS - 1) / HG_LN_ROWS;
  const size_t pa = (size_t)ncs * w.ldg, pb = (size_t)nln * 3 * DM;
  w.Z = take((size_t)rows * DM * sizeof(float));
  w.H = take((size_t)rows * DM * sizeof(float));
  w.dH = take((size_t)rows * DM * sizeof(float));
  w.G = take((size_t)w.chunk_rows * w.ldg * sizeof(float));
  w.slab = take((size_t)nslab * wide * DM * sizeof(float));
  w.part = take((pa > pb ? pa : pb) * sizeof(float));
  w.bytes = off;
  return w;
}

int launch_head_grads(const HeadGradArgs& a, hipStream_t st) {
  const long rows = (long)a.B * a.Tq * a.A;
  if (rows <= 0 || rows > 0x7fffffffL / (3 * DM)) return CTRLSIM_EINVAL;
  if (!a.X || !a.exist || !a.st12 || !a.sums || !a.grads || !a.Z || !a.H || !a.dH || !a.G || !a.slab || !a.part ||
      a.chunk_rows < 1 || (a.ldg & 3))
    return CTRLSIM_EINVAL;
  const HgRowCtx rc{a.exist, a.moving, a.sums, a.Tq, a.A, a.supervise_moving, rows};
  if (a.dX && hipMemsetAsync(a.dX, 0, (size_t)rows * 3 * DM * sizeof(float), st) != hipSuccess) return CTRLSIM_ELAUNCH;
  bool touched[3] = {false, false, false};
  for (int hi = 0; hi < a.nheads; ++hi) {
    const HeadGradHead& h = a.h[hi];
    const int width = h.n * h.nsm;
    if (!h.w0 || !h.b0 || !h.g || !h.be || !h.w3 || !h.b3 || h.k < 0 || h.k > 2 || h.nsm < 1 || h.nsm > 3 || width < 1 || width > a.ldg)
      return CTRLSIM_EINVAL;
    float* g = a.grads + h.goff;                       // mlp.0.weight, mlp.0.bias, mlp.1.weight, mlp.1.bias, mlp.3.weight, mlp.3.bias
    float *gW0 = g, *gb0 = gW0 + DM * DM, *gg = gb0 + DM, *gbe = gg + DM, *gW3 = gbe + DM, *gb3 = gW3 + (long)width * DM;
    const float* Xk = a.X + h.k * DM;
    // Z = X_k W0^T + b0, H = relu(LN(Z))
    HG_CHK(hg_gemm(1, 1, HgGemm{Xk, 3 * DM, 1, h.w0, 1, DM, a.Z, DM, 0, h.b0, (int)rows, DM, DM, DM, 0}, st));
    hipLaunchKernelGGL(hg_ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a.Z, h.g, h.be, a.H, rows);
    int nslab = 0, ncs = 0;
    for (long r0 = 0; r0 < rows; r0 += a.chunk_rows) {
      const int nr = (int)(rows - r0 < a.chunk_rows ? rows - r0 : a.chunk_rows);
      const float* Hc = a.H + r0 * DM;
      // Y -> G in place
      HG_CHK(hg_gemm(1, 1, HgGemm{Hc, DM, 1, h.w3, 1, DM, a.G, a.ldg, 0, h.b3, nr, width, DM, DM, 0}, st));
      if (h.kind == 2)
        hipLaunchKernelGGL(hg_g_state_kernel, dim3((unsigned)(((long)nr * a.nfut + 255) / 256)), dim3(256), 0, st, a.G, (long)a.ldg, a.nfut,
                           r0, nr, a.st12, a.local_frame, rc);
      else
        hipLaunchKernelGGL(hg_g_ce_kernel, dim3((nr + 3) / 4), dim3(256), 0, st, a.G, (long)a.ldg, h.n, h.nsm, r0, nr, h.sm0, h.tgt,
                           h.kind == 0 ? a.shift : 0L, h.kind == 0, h.kind == 0 ? a.action_coef : 1.0f, rc);
      // dH = G W3 (all classes inside one workgroup)
      HG_CHK(hg_gemm(1, 0, HgGemm{a.G, a.ldg, 1, h.w3, DM, 1, a.dH + r0 * DM, DM, 0, nullptr, nr, DM, width, width, 0}, st));
      // dW3 partial slabs = G^T H over blocks of HG_KS rows; db3 partials
      HG_CHK(hg_gemm(0, 0, HgGemm{a.G, 1, a.ldg, Hc, DM, 1, a.slab + (long)nslab * width * DM, DM, (long)width * DM, nullptr, width, DM, nr,
                                  HG_KS, 0}, st));
      nslab += (nr + HG_KS - 1) / HG_KS;
      const int nb = (nr + HG_CS_ROWS - 1) / HG_CS_ROWS;
      hipLaunchKernelGGL(hg_colsum_kernel, dim3((width + 255) / 256, nb), dim3(256), 0, st, a.G, (long)a.ldg, nr, width,
                         a.part + (long)ncs * width);
      ncs += nb;
    }
    HG_CHK(hg_reduce(a.slab, nslab, (long)width * DM, (long)width * DM, gW3, st));
    HG_CHK(hg_reduce(a.part, ncs, width, width, gb3, st));
    // ReLU + LayerNorm backward: dH -> dZ in place, partials of dgamma, dbeta, db0
    const int nln = (int)((rows + HG_LN_ROWS - 1) / HG_LN_ROWS);
    hipLaunchKernelGGL(hg_ln_bwd_kernel, dim3(nln), dim3(256), 0, st, a.Z, h.g, h.be, a.dH, rows, a.part);
    HG_CHK(hg_reduce(a.part, nln, 3 * DM, DM, gg, st));
    HG_CHK(hg_reduce(a.part + DM, nln, 3 * DM, DM, gbe, st));
    HG_CHK(hg_reduce(a.part + 2 * DM, nln, 3 * DM, DM, gb0, st));
    // dW0 = dZ^T X_k
    HG_CHK(hg_gemm(0, 0, HgGemm{a.dH, 1, DM, Xk, 3 * DM, 1, a.slab, DM, (long)DM * DM, nullptr, DM, DM, (int)rows, HG_KS, 0}, st));
    HG_CHK(hg_reduce(a.slab, (int)((rows + HG_KS - 1) / HG_KS), (long)DM * DM, (long)DM * DM, gW0, st));
    // dX_k (+)= dZ W0
    if (a.dX) {
      HG_CHK(hg_gemm(1, 0, HgGemm{a.dH, DM, 1, h.w0, DM, 1, a.dX + h.k * DM, 3 * DM, 0, nullptr, (int)rows, DM, DM, DM, touched[h.k] ? 1 : 0}, st));
      touched[h.k] = true;
    }
  }
  return ctrlsim_launch_status();
}
