// Graph attention over the nodes of each segment (GraphAttentionLayer,
// reference sgan/models.py:184-220; ELU / log_softmax of GAT.forward :236-237).
//
// The reference builds the (N, N, 2F) concatenation [Wh_i || Wh_j] and
// multiplies it by `a` (models.py:212-220): e_ij = a1.Wh_i + a2.Wh_j.  We use
// that decomposition directly (s_i + t_j, 2NF MACs instead of 2N^2F), which
// is exact up to fp32 reassociation.  One workgroup (4 waves) per segment
// (scene for the intra-group graph, the scene's groups for the inter-group
// graph); Wh is LDS-resident (odd row stride), the attention of a 16-row
// block lives in registers and both products (att @ Wh, and the backward's
// dhp @ Wh^T / att^T @ dhp) run on fp32 MFMA tiles (below).
//
// Multi-head (the batched GAT of the sgangat family, sgan/GAT.py:6-55 text):
// Wh holds all heads side by side (n x heads*F, the output of one X @ [w_0 |
// .. | w_{H-1}] transform), `a` is heads x [a_src | a_dst], and the workgroup
// grid runs over (segment, head) pairs; head h writes columns [hF, hF + F) of
// y, so the concatenation of heads (GAT.py:86) is free.  `bias` (F, shared by
// the heads, GAT.py:41) is added to the aggregate before the epilogue.
#include "gat_common.h"
#include "dropout_common.h"

namespace sgg {

// phase timestamps of workgroup 0's first (segment, head) (tools/gat_layer_probe.hip)
#ifdef SGG_GAT_PROF
__device__ long long g_gat_prof[64];
#define GPMARK(i) \
  if (threadIdx.x == 0 && blockIdx.x == 0) g_gat_prof[i] = wall_clock64();
#else
#define GPMARK(i)
#endif

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Both kernels work on 16 x 16 x 4 fp32 MFMA tiles (exact fp32 products;
// v_mfma_f32_16x16x4_f32: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][c
// = lane & 15], C rows 4 (lane >> 4) + v, column lane & 15).  One workgroup
// per (segment, head); wave w takes the 16-node row blocks w, w + 4, ...
//
// Forward: the attention rows of a row block are built directly in the A
// operand layout (lane = row i, k-step m = nodes 4m + (lane >> 4)), so the
// softmax needs two cross-lane steps per reduction and the aggregation
// att @ Wh reads only Wh (LDS) -- no attention matrix is stored.

// softmax attention + aggregation + bias + epilogue of one (segment, head)
// from the LDS tile Ws (nr x Fs, zero rows past n) and its scores.  DROP:
// attention dropout (dk: the (site, head)'s mask key, dropout_common.h) on the
// normalised attention -- row o + i of the node array, in-segment column j
template <int NM, bool DROP = false>
__device__ __forceinline__ void gat_attend(const float* Ws, int Fs, const float* ss, const float* ts,
                                           const float* lab, int o, int n, int nr, int F, int HF, int c0, float alpha,
                                           int mode, int epi, const float* __restrict__ bias, float* __restrict__ hp,
                                           float* __restrict__ y, int ldy, const DropKey dk = DropKey{}) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int nct = (F + 15) >> 4;
  const int nm = nr >> 2;
  for (int rb = wave; 16 * rb < n; rb += kGatWaves) {
    const int i = 16 * rb + r16;
    const bool iv = i < n;
    const float si = ss[i], li = lab[i];
    float p[NM];
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      p[m] = -INFINITY;
      if (m < nm) {
        const int j = 4 * m + q;
        const bool edge = iv && j < n && (mode == 1 || i == j || (li != 0.f && li == lab[j]));
        if (edge) {
          p[m] = lrelu(si + ts[j], alpha);
          mx = fmaxf(mx, p[m]);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const float e = p[m] == -INFINITY ? 0.f : expf(p[m] - mx);
      p[m] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = iv ? 1.f / sum : 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) p[m] *= inv;
    if constexpr (DROP) {
#pragma unroll
      for (int m = 0; m < NM; ++m)
        if (m < nm) p[m] = drop_word(dk, (uint32_t)(o + i), (uint32_t)(4 * m + q)) >= dk.thr ? p[m] * dk.scale : 0.f;
    }
    // out = att @ Wh (+ bias), 16-feature column tiles
    floatx4 hv[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      hv[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (ct < nct) {
        const int fb = min(16 * ct + r16, F - 1);
#pragma unroll
        for (int m = 0; m < NM; ++m)
          if (m < nm) hv[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[m], Ws[(4 * m + q) * Fs + fb], hv[ct], 0, 0, 0);
        const float bv = (bias && 16 * ct + r16 < F) ? bias[16 * ct + r16] : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) hv[ct][v] += bv;
      }
    }
    // epilogue per output row 16 rb + 4 q + v, feature 16 ct + r16
    SGG_GAT_EPILOGUE_STORE(16 * rb)
  }
}

// gat_fwd_kernel<NM> / gat_bwd_kernel<NJT> and their forms with attention
// dropout, gat_fwd_drop_kernel<NM> / gat_bwd_drop_kernel<NJT>: one text
// (gat_kernels.h) compiled twice -- with the body as a shared device function
// the kernels without dropout compile to other instruction streams
#define SGG_GAT_DROP 0
#include "gat_kernels.h"
#undef SGG_GAT_DROP
#define SGG_GAT_DROP 1
#include "gat_kernels.h"
#undef SGG_GAT_DROP

// One batched-GAT layer of the sgangat family in one launch (GAT.py:71-86
// text: InstanceNorm1d over the scene's nodes, then the multi-head attention
// layer): per (segment, head) the segment's input rows (one or two column
// blocks: [h | pool_h] without a concatenation) are staged in LDS, normalised
// per feature (the two-pass fp64 statistics of seg_norm_fwd_kernel, norm.hip,
// same row phases and combine order), transformed by the head's W (K x F, the
// module's (heads, K, F) layout: no permuted copy) on the MFMA -- fp32 16x16x4,
// or bf16 16x16x32 with xw_bf16_kernel's rounding and k order -- and attended.
// When saving (training), head 0 writes the normalised rows and 1 / std and
// every head its Wh block: the backward's operands.
struct GatLayerArgs {
  const float *x1, *x2;
  int ld1, K1, ld2, K2;
  const float *w, *a_src, *a_dst, *bias;
  const int32_t* seg_off;
  int nseg, nrows, heads, F, epi, max_seg;
  float alpha, eps;
  float *xn, *rstd, *wh, *hp, *y;
  int ldy;
};

__host__ __device__ __forceinline__ int gat_layer_kp(int K) { return (K + 31) & ~31; }

// the layer over one set: workgroups blk = 0 .. nblk - 1 of those serving it
template <int NM, bool BF16>
__device__ __forceinline__ void gat_layer_fwd_body(const GatLayerArgs& p, int blk, int nblk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int F = p.F, K = p.K1 + p.K2, HF = p.heads * F;
  const int Fs = gat_fs(F);
  const int Kp = gat_layer_kp(K), Ks = Kp + 1;
  const int F16 = (F + 15) & ~15, Wp = F16 + 1;
  const int nmax = gat_r16(p.max_seg);
  GPMARK(0);
  // the first work item's offsets with the total (independent loads)
  const int gfirst = min(blk / p.heads, p.nseg);
  const int tot = p.seg_off[p.nseg], ofirst = p.seg_off[gfirst], efirst = p.seg_off[min(gfirst + 1, p.nseg)];
  gat_zero_pad_rows(tot, p.nrows, HF, p.y, p.ldy, p.epi ? p.hp : nullptr, blk, nblk);
  if (p.wh) {   // the saved operands too (the backward's products run over all rows)
    gat_zero_pad_rows(tot, p.nrows, HF, p.wh, HF, nullptr, blk, nblk);
    gat_zero_pad_rows(tot, p.nrows, K, p.xn, K, nullptr, blk, nblk);
  }
  double(*red)[64] = reinterpret_cast<double(*)[64]>(smem);   // 8 x 64
  float* Xs = reinterpret_cast<float*>(smem + 8 * 64 * sizeof(double));   // nmax x Ks
  float* Wl = Xs + nmax * Ks;                   // Kp x Wp
  float* Ws = Wl + Kp * Wp;                     // nmax x Fs
  float* ss = Ws + nmax * Fs;
  float* ts = ss + nmax;
  float* lab = ts + nmax;
  float* al = lab + nmax;                       // 3F: the head's a_src | a_dst, the bias
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int fl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  for (int gh = blk; gh < p.nseg * p.heads; gh += nblk) {
    const int g = gh / p.heads, hd = gh - g * p.heads;
    const int o = gh == blk ? ofirst : p.seg_off[g];
    const int n = min((gh == blk ? efirst : p.seg_off[g + 1]) - o, nmax);   // (LDS plan bound)
    if (n <= 0) continue;
    const int c0 = hd * F;
    const int nr = gat_r16(n);
    const bool save = p.wh != nullptr;
    GPMARK(1);
    const float* wg = p.w + (size_t)hd * K * F;
    float av = 0.f;   // thread t < 3F: a_src | a_dst | bias entry t (issued with the tiles' loads)
    {
      const int t = threadIdx.x;
      if (t < F) av = p.a_src[(size_t)F * hd + t];
      else if (t < 2 * F) av = p.a_dst[(size_t)F * hd + t - F];
      else if (t < 3 * F && p.bias) av = p.bias[t - 2 * F];
    }
    stage_block(
        nr, Kp, n, K,
        [&](int r, int k) {
          return k < p.K1 ? p.x1[(size_t)(o + r) * p.ld1 + k] : p.x2[(size_t)(o + r) * p.ld2 + (k - p.K1)];
        },
        [&](int r, int k, float v) { Xs[r * Ks + k] = v; });
    stage_block(Kp, F16, K, F, [&](int k, int f) { return wg[(size_t)k * F + f]; },
                [&](int k, int f, float v) { Wl[k * Wp + f] = v; });
    if ((int)threadIdx.x < 3 * F) al[threadIdx.x] = av;
    for (int t = threadIdx.x + kGatThreads; t < 3 * F; t += kGatThreads)   // (F > 85)
      al[t] = t < F ? p.a_src[(size_t)F * hd + t] : t < 2 * F ? p.a_dst[(size_t)F * hd + t - F]
                                                             : (p.bias ? p.bias[t - 2 * F] : 0.f);
    __syncthreads();
    GPMARK(2);
    // instance norm per feature over the segment's rows (in place)
    // (one pass: fp64 sum and sum of squares -- exact enough for fp32 data
    // that var = E[x^2] - mean^2 loses nothing at fp32 -- two chains each)
    for (int f0 = 0; f0 < K; f0 += 64) {
      const int f = f0 + fl;
      const bool fok = f < K;
      double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
      if (fok) {
        int r = ph;
        for (; r + 4 < n; r += 8) {
          const double x0 = Xs[r * Ks + f], x1 = Xs[(r + 4) * Ks + f];
          s0 += x0;
          s1 += x1;
          q0 = fma(x0, x0, q0);
          q1 = fma(x1, x1, q1);
        }
        if (r < n) {
          const double x0 = Xs[r * Ks + f];
          s0 += x0;
          q0 = fma(x0, x0, q0);
        }
      }
      red[ph][fl] = s0 + s1;
      red[4 + ph][fl] = q0 + q1;
      __syncthreads();
      const double meand = ((red[0][fl] + red[1][fl]) + (red[2][fl] + red[3][fl])) / n;
      const double sq = ((red[4][fl] + red[5][fl]) + (red[6][fl] + red[7][fl])) / n;
      __syncthreads();
      const float mean = (float)meand;
      const double vard = sq - meand * meand;
      const float rs = 1.f / sqrtf((float)(vard > 0.0 ? vard : 0.0) + p.eps);
      if (fok) {
        for (int r = ph; r < n; r += 4) {
          const float v = (Xs[r * Ks + f] - mean) * rs;
          Xs[r * Ks + f] = v;
          if (save && hd == 0) p.xn[(size_t)(o + r) * K + f] = v;
        }
        if (save && hd == 0 && ph == 0) p.rstd[(size_t)g * K + f] = rs;
      }
    }
    __syncthreads();
    GPMARK(3);
    // Wh = Xn W_h: (row block, column tile) MFMA tiles over the waves
    const int nrb = nr >> 4, nct = F16 >> 4;
    for (int tile = wave; tile < nrb * nct; tile += kGatWaves) {
      const int rb = tile / nct, ct = tile - rb * nct;
      floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
      const float* xr = Xs + (16 * rb + r16) * Ks;
      if constexpr (BF16) {
        for (int k0 = 0; k0 < Kp; k0 += 32) {
          const int kb = k0 + 8 * q;
          bf16x8 a, b;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            a[j] = (__bf16)xr[kb + j];
            b[j] = (__bf16)Wl[(kb + j) * Wp + 16 * ct + r16];
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
      } else {
        for (int k0 = 0; k0 < K; k0 += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[k0 + q], Wl[(k0 + q) * Wp + 16 * ct + r16], acc, 0, 0, 0);
      }
      const int f = 16 * ct + r16;
      if (f < F) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * rb + 4 * q + v;
          Ws[r * Fs + f] = acc[v];
          if (save && r < n) p.wh[(size_t)(o + r) * HF + c0 + f] = acc[v];
        }
      }
    }
    __syncthreads();
    GPMARK(4);
    gat_scores(Ws, Fs, al, al + F, F, nullptr, 1, o, n, nr, ss, ts, lab);
    __syncthreads();
    GPMARK(5);
    gat_attend<NM>(Ws, Fs, ss, ts, lab, o, n, nr, F, HF, c0, p.alpha, 1, p.epi, p.bias ? al + 2 * F : nullptr, p.hp,
                   p.y, p.ldy);
    GPMARK(6);
    __syncthreads();  // LDS reused by the next segment
    GPMARK(7);
  }
}

template <int NM, bool BF16>
__global__ void __launch_bounds__(kGatThreads) gat_layer_fwd_kernel(const GatLayerArgs p) {
  gat_layer_fwd_body<NM, BF16>(p, blockIdx.x, gridDim.x);
}

// two sets (batches) through the same layer weights in one launch
// (sgg_gat_layer_fwd2): workgroups [0, g1) serve set a, [g1, grid) set b
template <int NM, bool BF16>
__global__ void __launch_bounds__(kGatThreads) gat_layer_fwd2_kernel(const GatLayerArgs a, const GatLayerArgs b, int g1) {
  if ((int)blockIdx.x < g1)
    gat_layer_fwd_body<NM, BF16>(a, blockIdx.x, g1);
  else
    gat_layer_fwd_body<NM, BF16>(b, blockIdx.x - g1, gridDim.x - g1);
}

static size_t gat_layer_lds(int K, int F, int max_seg) {
  const size_t nm = gat_r16(max_seg), Kp = gat_layer_kp(K);
  return 8 * 64 * sizeof(double) +
         sizeof(float) * (nm * (Kp + 1) + Kp * (((F + 15) & ~15) + 1) + nm * gat_fs(F) + 3 * nm + 3 * F) + 16;
}

// da_src / da_dst (heads x F each) and dbias (F, summed over the heads) from
// the (segment, head) partials of gat_bwd_kernel: one workgroup per output,
// a fixed-order fp64 tree over the segments
__global__ void __launch_bounds__(256) gat_param_reduce_kernel(const float* __restrict__ pda,
                                                               const double* __restrict__ pdb, int nseg, int heads,
                                                               int F, float* __restrict__ da_src,
                                                               float* __restrict__ da_dst, float* __restrict__ dbias) {
  __shared__ double red[256];
  const int e = blockIdx.x, na = heads * 2 * F;
  const int t = threadIdx.x;
  double acc = 0.0;
  if (e < na) {
    const int h = e / (2 * F), c = e - h * 2 * F;
    for (int g = t; g < nseg; g += 256) acc += (double)pda[((size_t)g * heads + h) * 2 * F + c];
  } else {
    const int f = e - na;
    for (int gh = t; gh < nseg * heads; gh += 256) acc += pdb[(size_t)gh * F + f];
  }
  red[t] = acc;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (t < s2) red[t] += red[t + s2];
    __syncthreads();
  }
  if (t == 0) {
    if (e < na) {
      const int h = e / (2 * F), c = e - h * 2 * F;
      if (c < F) da_src[h * F + c] = (float)red[0];
      else da_dst[h * F + c - F] = (float)red[0];
    } else {
      dbias[e - na] = (float)red[0];
    }
  }
}

// (rows: slab rows of heads partials each -- the segments of gat_bwd_kernel,
// the column units of gat_wide.hip)
void gat_param_reduce(const float* pda, const double* pdb, int rows, int heads, int F, float* da_src, float* da_dst,
                      float* dbias, hipStream_t st) {
  hipLaunchKernelGGL(gat_param_reduce_kernel, dim3(heads * 2 * F + (dbias ? F : 0)), dim3(256), 0, st, pda, pdb, rows,
                     heads, F, da_src, da_dst, dbias);
}

static size_t gat_fwd_lds(int F, int max_seg) {
  const size_t nm = gat_r16(max_seg);
  return sizeof(float) * (nm * gat_fs(F) + 3 * nm + 2 * F) + 16;
}
static size_t gat_bwd_lds(int F, int max_seg) {
  const size_t nm = gat_r16(max_seg);
  return sizeof(float) * (2 * nm * gat_fs(F) + nm * (nm + 4) + 6 * nm + (nm / 16) * nm + 2 * F) + 16;
}

}  // namespace sgg

using namespace sgg;

static int gat_args_ok(const char* who, const float* Wh, int heads, const float* a, const float* labels,
                       const int32_t* off, int nseg, int n, int F, int mode, int epi, int max_seg) {
  SGG_CHECK_ARG(Wh && a && off, "%s: null pointer", who);
  SGG_CHECK_ARG(mode == 1 || labels, "%s: mask_mode 0 needs labels", who);
  SGG_CHECK_ARG(nseg >= 0 && n >= 0, "%s: bad sizes", who);
  SGG_CHECK_ARG(F >= 1 && F <= 128, "%s: F=%d outside [1, 128]", who, F);
  SGG_CHECK_ARG(heads >= 1 && heads <= 64, "%s: heads=%d outside [1, 64]", who, heads);
  SGG_CHECK_ARG(mode == 0 || mode == 1, "%s: bad mask_mode", who);
  SGG_CHECK_ARG(epi >= 0 && epi <= 2, "%s: bad epilogue", who);
  SGG_CHECK_ARG(epi != 2 || heads == 1, "%s: the log_softmax epilogue is single-head", who);
  SGG_CHECK_ARG(max_seg >= 1 && max_seg <= SGG_GAT_MAX_NODES, "%s: max segment %d outside [1, %d]", who, max_seg,
                SGG_GAT_MAX_NODES);
  return 0;
}

static int gat_grid(int nseg, int heads) {
  const long long w = (long long)nseg * heads;
  return w < 1 ? 1 : w < 16384 ? (int)w : 16384;
}

static int gat_fwd_launch(const char* who, const float* Wh, int heads, const float* as, const float* ad, int lda,
                          const float* bias, const float* labels, const int32_t* seg_off, int nseg, int n, int F,
                          float alpha, int mask_mode, int epilogue, int max_seg, float* hp, float* y, int ldy,
                          void* stream, const DropArgs* drop = nullptr) {
  int rc = gat_args_ok(who, Wh, heads, as, labels, seg_off, nseg, n, F, mask_mode, epilogue, max_seg);
  if (rc) return rc;
  SGG_CHECK_ARG(ad, "%s: null a_dst", who);
  SGG_CHECK_ARG(y && (epilogue == 0 || hp), "%s: null output", who);
  SGG_CHECK_ARG(ldy >= heads * F, "%s: ldy < heads * F", who);
  SGG_CHECK_ARG(epilogue != 2 || ldy == F, "%s: log_softmax epilogue needs a dense y (ldy == F)", who);
  if (nseg == 0 && n == 0) return 0;   // (rows but no segments: the kernel zeroes the rows)
  if (drop) {
    auto kd = max_seg <= 32 ? gat_fwd_drop_kernel<8> : max_seg <= 64 ? gat_fwd_drop_kernel<16>
                                                                       : gat_fwd_drop_kernel<32>;
    hipLaunchKernelGGL(kd, dim3(gat_grid(nseg, heads)), dim3(kGatThreads), gat_fwd_lds(F, max_seg),
                       (hipStream_t)stream, Wh, heads, as, ad, lda, bias, labels, seg_off, nseg, n, F, alpha,
                       mask_mode, epilogue, max_seg, hp, y, ldy, *drop);
    SGG_RETURN_LAUNCH(who);
  }
  auto k = max_seg <= 32 ? gat_fwd_kernel<8> : max_seg <= 64 ? gat_fwd_kernel<16> : gat_fwd_kernel<32>;
  hipLaunchKernelGGL(k, dim3(gat_grid(nseg, heads)), dim3(kGatThreads), gat_fwd_lds(F, max_seg), (hipStream_t)stream,
                     Wh, heads, as, ad, lda, bias, labels, seg_off, nseg, n, F, alpha, mask_mode, epilogue, max_seg,
                     hp, y, ldy);
  SGG_RETURN_LAUNCH(who);
}

static int gat_bwd_launch(const char* who, const float* Wh, int heads, const float* as, const float* ad, int lda,
                          const float* labels, const int32_t* seg_off, int nseg, int n, int F, float alpha,
                          int mask_mode, int epilogue, int max_seg, const float* hp, const float* y, const float* dy,
                          int lddy, float* dWh, float* ds, float* dt, float* pda, double* pdb, void* stream,
                          const DropArgs* drop = nullptr) {
  int rc = gat_args_ok(who, Wh, heads, as, labels, seg_off, nseg, n, F, mask_mode, epilogue, max_seg);
  if (rc) return rc;
  SGG_CHECK_ARG(ad && dy && dWh, "%s: null pointer", who);
  SGG_CHECK_ARG(epilogue == 0 || hp, "%s: epilogue needs hp", who);
  SGG_CHECK_ARG(epilogue != 2 || y, "%s: log_softmax epilogue needs y", who);
  SGG_CHECK_ARG(lddy >= heads * F, "%s: lddy < heads * F", who);
  if (nseg == 0 && n == 0) return 0;
  const size_t lds = gat_bwd_lds(F, max_seg);
  SGG_CHECK_ARG(lds <= 160 * 1024, "%s: segment %d x F %d needs %zu B of LDS", who, max_seg, F, lds);
  if (drop) {
    auto kd = max_seg <= 32 ? gat_bwd_drop_kernel<2> : max_seg <= 64 ? gat_bwd_drop_kernel<4>
                                                                      : gat_bwd_drop_kernel<8>;
    hipLaunchKernelGGL(kd, dim3(gat_grid(nseg, heads)), dim3(kGatThreads), lds, (hipStream_t)stream, Wh, heads, as,
                       ad, lda, labels, seg_off, nseg, n, F, alpha, mask_mode, epilogue, max_seg, hp, y, dy, lddy,
                       dWh, ds, dt, pda, pdb, *drop);
    SGG_RETURN_LAUNCH(who);
  }
  auto k = max_seg <= 32 ? gat_bwd_kernel<2> : max_seg <= 64 ? gat_bwd_kernel<4> : gat_bwd_kernel<8>;
  hipLaunchKernelGGL(k, dim3(gat_grid(nseg, heads)), dim3(kGatThreads), lds, (hipStream_t)stream, Wh, heads, as, ad,
                     lda, labels, seg_off, nseg, n, F, alpha, mask_mode, epilogue, max_seg, hp, y, dy, lddy, dWh, ds,
                     dt, pda, pdb);
  SGG_RETURN_LAUNCH(who);
}

extern "C" int sgg_gat_fwd(const float* Wh, int heads, const float* a, const float* bias, const float* labels,
                           const int32_t* seg_off, int nseg, int n, int F, float alpha, int mask_mode, int epilogue,
                           int max_seg, float* hp, float* y, int ldy, void* stream) {
  return gat_fwd_launch("sgg_gat_fwd", Wh, heads, a, a ? a + F : nullptr, 2 * F, bias, labels, seg_off, nseg, n, F,
                        alpha, mask_mode, epilogue, max_seg, hp, y, ldy, stream);
}

extern "C" int sgg_gat_bwd(const float* Wh, int heads, const float* a, const float* labels, const int32_t* seg_off,
                           int nseg, int n, int F, float alpha, int mask_mode, int epilogue, int max_seg,
                           const float* hp, const float* y, const float* dy, int lddy, float* dWh, float* ds,
                           float* dt, void* stream) {
  SGG_CHECK_ARG(ds && dt, "sgg_gat_bwd: null pointer");
  return gat_bwd_launch("sgg_gat_bwd", Wh, heads, a, a ? a + F : nullptr, 2 * F, labels, seg_off, nseg, n, F, alpha,
                        mask_mode, epilogue, max_seg, hp, y, dy, lddy, dWh, ds, dt, nullptr, nullptr, stream);
}

static size_t gat_pda_bytes(int nseg, int heads, int F) {
  return ((size_t)nseg * heads * 2 * F * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" size_t sgg_gat_bwd_ex_work_bytes(int nseg, int heads, int F) {
  if (nseg < 0 || heads < 1 || F < 1) return 0;
  return gat_pda_bytes(nseg, heads, F) + (size_t)nseg * heads * F * sizeof(double);
}

extern "C" int sgg_gat_fwd_ex(const float* Wh, int heads, const float* a_src, const float* a_dst, const float* bias,
                              const float* labels, const int32_t* seg_off, int nseg, int n, int F, float alpha,
                              int mask_mode, int epilogue, int max_seg, float* hp, float* y, int ldy, void* stream) {
  return gat_fwd_launch("sgg_gat_fwd_ex", Wh, heads, a_src, a_dst, F, bias, labels, seg_off, nseg, n, F, alpha,
                        mask_mode, epilogue, max_seg, hp, y, ldy, stream);
}

extern "C" int sgg_gat_bwd_ex(const float* Wh, int heads, const float* a_src, const float* a_dst, const float* labels,
                              const int32_t* seg_off, int nseg, int n, int F, float alpha, int mask_mode, int epilogue,
                              int max_seg, const float* hp, const float* y, const float* dy, int lddy, float* dWh,
                              float* da_src, float* da_dst, float* dbias, void* work, void* stream) {
  SGG_CHECK_ARG(da_src && da_dst && work, "sgg_gat_bwd_ex: null pointer");
  SGG_CHECK_ARG(((uintptr_t)work & 15) == 0, "sgg_gat_bwd_ex: work must be 16-byte aligned");
  float* pda = reinterpret_cast<float*>(work);
  double* pdb = dbias ? reinterpret_cast<double*>(reinterpret_cast<char*>(work) + gat_pda_bytes(nseg, heads, F))
                      : nullptr;
  int rc = gat_bwd_launch("sgg_gat_bwd_ex", Wh, heads, a_src, a_dst, F, labels, seg_off, nseg, n, F, alpha, mask_mode,
                          epilogue, max_seg, hp, y, dy, lddy, dWh, nullptr, nullptr, pda, pdb, stream);
  if (rc) return rc;
  // (no segments: the reduce writes zero gradients)
  gat_param_reduce(pda, pdb, nseg, heads, F, da_src, da_dst, dbias, (hipStream_t)stream);
  SGG_RETURN_LAUNCH("sgg_gat_bwd_ex");
}

// the dropout arguments of an entry point -> DropArgs (thr / scale computed
// here, once); the limits of the mask contract (include/sgg.h)
static int gat_drop_args(const char* who, float p, unsigned long long seed, unsigned offset, unsigned site,
                         unsigned head0, int heads, const unsigned long long* rng_dev, DropArgs* out) {
  SGG_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout p=%g outside [0, 1)", who, (double)p);
  SGG_CHECK_ARG(site < (1u << 24), "%s: dropout site %u is not below 2^24", who, site);
  SGG_CHECK_ARG(head0 < 256u && head0 + (unsigned)heads <= 256u, "%s: dropout heads %u + %d above 256", who, head0,
                heads);
  SGG_CHECK_ARG(((uintptr_t)rng_dev & 7) == 0, "%s: rng_dev must be 8-byte aligned", who);
  *out = DropArgs{seed, rng_dev, offset, site, head0, drop_threshold(p), drop_scale(p)};
  return 0;
}

extern "C" int sgg_gat_fwd_drop(const float* Wh, int heads, const float* a_src, const float* a_dst, int lda,
                                const float* bias, const float* labels, const int32_t* seg_off, int nseg, int n,
                                int F, float alpha, int mask_mode, int epilogue, int max_seg, float* hp, float* y,
                                int ldy, float p, unsigned long long seed, unsigned offset, unsigned site,
                                unsigned head0, const unsigned long long* rng_dev, void* stream) {
  const char* who = "sgg_gat_fwd_drop";
  SGG_CHECK_ARG(heads >= 1 && lda >= F, "%s: lda < F", who);
  DropArgs d;
  if (int rc = gat_drop_args(who, p, seed, offset, site, head0, heads, rng_dev, &d)) return rc;
  return gat_fwd_launch(who, Wh, heads, a_src, a_dst, lda, bias, labels, seg_off, nseg, n, F, alpha, mask_mode,
                        epilogue, max_seg, hp, y, ldy, stream, &d);
}

extern "C" int sgg_gat_bwd_drop(const float* Wh, int heads, const float* a_src, const float* a_dst, int lda,
                                const float* labels, const int32_t* seg_off, int nseg, int n, int F, float alpha,
                                int mask_mode, int epilogue, int max_seg, const float* hp, const float* y,
                                const float* dy, int lddy, float* dWh, float* ds, float* dt, float* da_src,
                                float* da_dst, float* dbias, void* work, float p, unsigned long long seed,
                                unsigned offset, unsigned site, unsigned head0, const unsigned long long* rng_dev,
                                void* stream) {
  const char* who = "sgg_gat_bwd_drop";
  SGG_CHECK_ARG(heads >= 1 && lda >= F, "%s: lda < F", who);
  SGG_CHECK_ARG((ds != nullptr) == (dt != nullptr), "%s: ds and dt go together", who);
  SGG_CHECK_ARG((da_src != nullptr) == (da_dst != nullptr) && (!dbias || da_src),
                "%s: da_src, da_dst (and dbias) go together", who);
  SGG_CHECK_ARG(!da_src || (work && ((uintptr_t)work & 15) == 0), "%s: da_src needs a 16-byte aligned work", who);
  DropArgs d;
  if (int rc = gat_drop_args(who, p, seed, offset, site, head0, heads, rng_dev, &d)) return rc;
  float* pda = da_src ? reinterpret_cast<float*>(work) : nullptr;
  double* pdb = dbias ? reinterpret_cast<double*>(reinterpret_cast<char*>(work) + gat_pda_bytes(nseg, heads, F))
                      : nullptr;
  int rc = gat_bwd_launch(who, Wh, heads, a_src, a_dst, lda, labels, seg_off, nseg, n, F, alpha, mask_mode, epilogue,
                          max_seg, hp, y, dy, lddy, dWh, ds, dt, pda, pdb, stream, &d);
  if (rc || !da_src) return rc;
  // (no segments: the reduce writes zero gradients)
  gat_param_reduce(pda, pdb, nseg, heads, F, da_src, da_dst, dbias, (hipStream_t)stream);
  SGG_RETURN_LAUNCH(who);
}

extern "C" size_t sgg_gat_layer_lds_bytes(int K, int F, int max_seg) {
  if (K < 1 || F < 1 || max_seg < 1) return 0;
  return gat_layer_lds(K, F, max_seg);
}

static int gat_layer_set_check(const SggGatLayerSet& s, int K, int HF, char which) {
  SGG_CHECK_ARG(s.x1 && s.seg_off && s.y && s.K1 >= 1 && s.ld1 >= s.K1 && (!s.x2 || (s.K2 >= 1 && s.ld2 >= s.K2)) &&
                    s.K1 + (s.x2 ? s.K2 : 0) == K && s.ldy >= HF && s.nseg >= 0 && s.n >= 0,
                "sgg_gat_layer_fwd2: bad set %c", which);
  SGG_CHECK_ARG(s.max_seg >= 1 && s.max_seg <= SGG_GAT_MAX_NODES, "sgg_gat_layer_fwd2: set %c max segment %d",
                which, s.max_seg);
  SGG_CHECK_ARG(!s.wh || (s.xn && s.rstd), "sgg_gat_layer_fwd2: set %c saves without xn / rstd", which);
  return 0;
}

extern "C" int sgg_gat_layer_fwd2(const SggGatLayerSet* sa, const SggGatLayerSet* sb, const float* w,
                                  const float* a_src, const float* a_dst, const float* bias, int heads, int F,
                                  float alpha, float eps, int epilogue, int bf16, void* stream) {
  SGG_CHECK_ARG(sa && sb && w && a_src && a_dst, "sgg_gat_layer_fwd2: null pointer");
  SGG_CHECK_ARG(F >= 1 && F <= 128 && heads >= 1 && heads <= 64, "sgg_gat_layer_fwd2: F=%d heads=%d", F, heads);
  SGG_CHECK_ARG(epilogue == 0 || epilogue == 1, "sgg_gat_layer_fwd2: epilogue must be 0 or 1");
  const int K = sa->K1 + (sa->x2 ? sa->K2 : 0);
  SGG_CHECK_ARG(K >= 1 && K <= 256, "sgg_gat_layer_fwd2: K=%d", K);
  if (int rc = gat_layer_set_check(*sa, K, heads * F, 'a')) return rc;
  if (int rc = gat_layer_set_check(*sb, K, heads * F, 'b')) return rc;
  SGG_CHECK_ARG(epilogue == 0 || (sa->hp && sb->hp), "sgg_gat_layer_fwd2: the ELU epilogue needs hp");
  // one LDS plan for both sets: the larger segment bound
  const int max_seg = sa->max_seg > sb->max_seg ? sa->max_seg : sb->max_seg;
  const size_t lds = gat_layer_lds(K, F, max_seg);
  SGG_CHECK_ARG(lds <= 160 * 1024, "sgg_gat_layer_fwd2: K %d, F %d, %d nodes need %zu B of LDS", K, F, max_seg, lds);
  auto args = [&](const SggGatLayerSet& s) {
    return GatLayerArgs{s.x1, s.x2, s.ld1, s.K1, s.ld2, s.x2 ? s.K2 : 0, w, a_src, a_dst, bias, s.seg_off, s.nseg,
                        s.n, heads, F, epilogue, max_seg, alpha, eps, s.xn, s.rstd, s.wh, s.hp, s.y, s.ldy};
  };
  const int g1 = gat_grid(sa->nseg, heads), g2 = gat_grid(sb->nseg, heads);
  auto k = bf16 ? (max_seg <= 32 ? gat_layer_fwd2_kernel<8, true> : max_seg <= 64 ? gat_layer_fwd2_kernel<16, true>
                                                                                   : gat_layer_fwd2_kernel<32, true>)
                : (max_seg <= 32 ? gat_layer_fwd2_kernel<8, false> : max_seg <= 64 ? gat_layer_fwd2_kernel<16, false>
                                                                                    : gat_layer_fwd2_kernel<32, false>);
  hipLaunchKernelGGL(k, dim3(g1 + g2), dim3(kGatThreads), lds, (hipStream_t)stream, args(*sa), args(*sb), g1);
  SGG_RETURN_LAUNCH("sgg_gat_layer_fwd2");
}

extern "C" int sgg_gat_layer_fwd(const float* x1, int ld1, int K1, const float* x2, int ld2, int K2, const float* w,
                                 const float* a_src, const float* a_dst, const float* bias, const int32_t* seg_off,
                                 int nseg, int n, int heads, int F, float alpha, float eps, int epilogue, int max_seg,
                                 int bf16, float* xn, float* rstd, float* wh, float* hp, float* y, int ldy,
                                 void* stream) {
  const int K = K1 + (x2 ? K2 : 0);
  SGG_CHECK_ARG(x1 && w && a_src && a_dst && seg_off && y, "sgg_gat_layer_fwd: null pointer");
  SGG_CHECK_ARG(K1 >= 1 && ld1 >= K1 && (!x2 || (K2 >= 1 && ld2 >= K2)), "sgg_gat_layer_fwd: bad input blocks");
  SGG_CHECK_ARG(K <= 256, "sgg_gat_layer_fwd: K=%d > 256", K);
  SGG_CHECK_ARG(F >= 1 && F <= 128 && heads >= 1 && heads <= 64, "sgg_gat_layer_fwd: F=%d heads=%d", F, heads);
  SGG_CHECK_ARG(epilogue == 0 || epilogue == 1, "sgg_gat_layer_fwd: epilogue must be 0 or 1");
  SGG_CHECK_ARG(epilogue == 0 || hp, "sgg_gat_layer_fwd: the ELU epilogue needs hp");
  SGG_CHECK_ARG(!wh || (xn && rstd), "sgg_gat_layer_fwd: saving needs xn, rstd and wh");
  SGG_CHECK_ARG(ldy >= heads * F && nseg >= 0 && n >= 0, "sgg_gat_layer_fwd: bad sizes");
  SGG_CHECK_ARG(max_seg >= 1 && max_seg <= SGG_GAT_MAX_NODES, "sgg_gat_layer_fwd: max segment %d outside [1, %d]",
                max_seg, SGG_GAT_MAX_NODES);
  const size_t lds = gat_layer_lds(K, F, max_seg);
  SGG_CHECK_ARG(lds <= 160 * 1024, "sgg_gat_layer_fwd: K %d, F %d, %d nodes need %zu B of LDS", K, F, max_seg, lds);
  if (nseg == 0 && n == 0) return 0;
  GatLayerArgs p{x1, x2, ld1, K1, ld2, x2 ? K2 : 0, w, a_src, a_dst, bias, seg_off, nseg, n, heads, F, epilogue,
                 max_seg, alpha, eps, xn, rstd, wh, hp, y, ldy};
  auto k = bf16 ? (max_seg <= 32 ? gat_layer_fwd_kernel<8, true> : max_seg <= 64 ? gat_layer_fwd_kernel<16, true>
                                                                                  : gat_layer_fwd_kernel<32, true>)
                : (max_seg <= 32 ? gat_layer_fwd_kernel<8, false> : max_seg <= 64 ? gat_layer_fwd_kernel<16, false>
                                                                                   : gat_layer_fwd_kernel<32, false>);
  hipLaunchKernelGGL(k, dim3(gat_grid(nseg, heads)), dim3(kGatThreads), lds, (hipStream_t)stream, p);
  SGG_RETURN_LAUNCH("sgg_gat_layer_fwd");
}
