// Graph attention for segments above SGG_GAT_MAX_NODES (up to
// SGG_GAT_WIDE_MAX_NODES) nodes: the pair space of a segment tiled, 64 rows
// per work unit against j (forward, backward rows) or 64 columns against i
// (backward columns) in tiles of 64 nodes.  Same semantics, operands and MFMA
// layouts as gat.hip, whose kernels hold a whole segment (and, backward, its
// attention matrix) in LDS; here nothing in LDS but the segment's t scores and
// labels (8 KiB at 1024 nodes) grows with the segment.
//
// The scores s, t and the softmax row statistics live in a caller-owned work
// buffer (sgg_gat_wide_work_floats) between the launches:
//   [ s | t | row max | row 1/sum | dot | ds ]   n x heads floats each (padded to 4)
//   [ pda: units x 2F floats | pdb: units x F doubles ]   the column units' partials
// (units = nseg x ceil(max_seg / 64) x heads).  The forward writes the first
// four, the backward reads them and writes the rest.
//
// A unit is (segment, 64-node block, head); the segment sizes may exist only
// on the device (the inter-group graph), so the grid is sized from max_seg and
// a unit whose block lies past its segment's end leaves at once.
#include "gat_common.h"

namespace sgg {

constexpr int kGwT = 64;                            // nodes per tile / rows per unit
constexpr int kGwMax = SGG_GAT_WIDE_MAX_NODES;
constexpr int kGwNa = kGwT + 4;                     // row stride of the attention tile (gat_bwd_kernel's Na)

__host__ __device__ __forceinline__ size_t gw_nh(int n, int heads) {
  const size_t v = (size_t)n * heads;
  return v < 4 ? 4 : (v + 3) & ~(size_t)3;
}
__host__ __device__ __forceinline__ int gw_blocks(int max_seg) { return (max_seg + kGwT - 1) / kGwT; }

// unit u -> (segment, block, head): heads fastest, so u indexes the partial
// slabs as gat_param_reduce reads them (row = segment x block)
struct GwUnit {
  int g, blk, hd;
};
__device__ __forceinline__ GwUnit gw_unit(long long u, int heads, int nblk) {
  const long long row = u / heads;
  return GwUnit{(int)(row / nblk), (int)(row % nblk), (int)(u - row * heads)};
}

// the segment's t scores and labels into LDS (rows [0, r16(n)), zero past n)
__device__ __forceinline__ void gw_stage_t(const float* __restrict__ t_in, const float* __restrict__ labels, int mode,
                                           int o, int n, int heads, int hd, float* ts, float* lab) {
  for (int j = threadIdx.x; j < gat_r16(n); j += kGatThreads) {
    ts[j] = j < n ? t_in[(size_t)(o + j) * heads + hd] : 0.f;
    lab[j] = (mode == 0 && j < n) ? labels[o + j] : 0.f;
  }
}

// ---- scores ---------------------------------------------------------------------
// s_i, t_i of every node and head through gat_scores' routine with the lane
// split the resident kernel uses for the node's whole segment: its bits.
__global__ void __launch_bounds__(kGatThreads) gat_wide_scores_kernel(
    const float* __restrict__ Wh, int heads, const float* __restrict__ a_src, const float* __restrict__ a_dst, int lda,
    const int32_t* __restrict__ seg_off, int nseg, int F, int max_seg, int nblk, float* __restrict__ s_out,
    float* __restrict__ t_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3, HF = heads * F;
  const int nmax = min(gat_r16(max_seg), kGwMax);
  float* Ws = reinterpret_cast<float*>(smem);   // kGwT x Fs
  float* ss = Ws + kGwT * Fs;
  float* ts = ss + kGwT;
  float* lab = ts + kGwT;
  float* al = lab + kGwT;                       // 2F: the head's a_src | a_dst
  const long long units = (long long)nseg * nblk * heads;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const GwUnit w = gw_unit(u, heads, nblk);
    const int o = seg_off[w.g];
    const int n = min(seg_off[w.g + 1] - o, nmax);
    const int i0 = kGwT * w.blk;
    if (i0 >= n) continue;
    const int ni = min(kGwT, n - i0), nrt = gat_r16(ni);
    const int c0 = w.hd * F;
    stage_block(nrt, F4, ni, F, [&](int r, int f) { return Wh[(size_t)(o + i0 + r) * HF + c0 + f]; },
                [&](int r, int f, float v) { Ws[r * Fs + f] = v; });
    for (int f = threadIdx.x; f < 2 * F; f += kGatThreads)
      al[f] = f < F ? a_src[(size_t)lda * w.hd + f] : a_dst[(size_t)lda * w.hd + f - F];
    __syncthreads();
    gat_scores(Ws, Fs, al, al + F, F, nullptr, 1, 0, ni, nrt, ss, ts, lab, nullptr, nullptr, gat_r16(n));
    __syncthreads();
    for (int r = threadIdx.x; r < ni; r += kGatThreads) {
      s_out[(size_t)(o + i0 + r) * heads + w.hd] = ss[r];
      t_out[(size_t)(o + i0 + r) * heads + w.hd] = ts[r];
    }
    __syncthreads();  // LDS reused by the next unit
  }
}

// ---- forward --------------------------------------------------------------------
// Unit = 64 rows of a (segment, head), 16 per wave in gat_attend's A-operand
// layout (lane = row i, k-step m = nodes 4m + (lane >> 4)).  The softmax runs
// in three sweeps over the segment's j with the exponentials recomputed: row
// max; row sum (each lane's partial in ascending k-step order, the xor 16 /
// xor 32 joins at the end); p * inv into the MFMA chain in ascending k-step
// order over Wh tiles of 64 nodes staged in LDS -- gat_attend's order of
// operations, so y and hp are its bits.  The next Wh tile is register-staged
// while the current one computes (NS: register slots per thread, F4 / 4
// rounded up to 8; every slot loads unconditionally, a clamped element past
// the tile, and is masked when stored -- a branch or a mask at the load would
// make the wave wait for each load in turn).  The row statistics are saved.
template <int NS>
__global__ void __launch_bounds__(kGatThreads) gat_fwd_wide_kernel(
    const float* __restrict__ Wh, int heads, const float* __restrict__ bias, const float* __restrict__ labels,
    const int32_t* __restrict__ seg_off, int nseg, int nrows, int F, float alpha, int mode, int epi, int max_seg,
    int nblk, const float* __restrict__ s_in, const float* __restrict__ t_in, float* __restrict__ rmax,
    float* __restrict__ rinv, float* __restrict__ hp, float* __restrict__ y, int ldy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3, HF = heads * F;
  const int nmax = min(gat_r16(max_seg), kGwMax);
  gat_zero_pad_rows(seg_off[nseg], nrows, HF, y, ldy, epi ? hp : nullptr);
  float* Wt = reinterpret_cast<float*>(smem);   // kGwT x Fs: the j tile of Wh
  float* ts = Wt + kGwT * Fs;                   // kGwMax
  float* lab = ts + kGwMax;                     // kGwMax
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int nct = (F + 15) >> 4;
  // a tile is 64 x F4 = 256 x (F4 / 4) elements: F4 / 4 <= 32 per thread
  const int nslot = F4 >> 2;
  const int tdq = kGatThreads / F4, tdr = kGatThreads - tdq * F4;
  const int tr0 = (int)threadIdx.x / F4, tc0 = (int)threadIdx.x - tr0 * F4;
  const long long units = (long long)nseg * nblk * heads;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const GwUnit w = gw_unit(u, heads, nblk);
    const int o = seg_off[w.g];
    const int n = min(seg_off[w.g + 1] - o, nmax);   // (clamped, memory-safe, as gat_fwd_kernel)
    const int i0 = kGwT * w.blk;
    if (i0 >= n) continue;
    const int hd = w.hd, c0 = hd * F;
    const int nm = gat_r16(n) >> 2;                  // k-steps of the segment
    const int ntile = (n + kGwT - 1) / kGwT;

    float treg[NS];
    int nj_ld = 0;   // valid rows of the register-staged tile
    auto tile_load = [&](int jb) {
      nj_ld = min(kGwT, n - jb);
      const float* base = Wh + (size_t)(o + jb) * HF + c0;
      int r = tr0, c = tc0;
#pragma unroll
      for (int e = 0; e < NS; ++e) {
        treg[e] = base[(size_t)min(r, nj_ld - 1) * HF + min(c, F - 1)];
        r += tdq;
        c += tdr;
        if (c >= F4) {
          c -= F4;
          ++r;
        }
      }
    };
    auto tile_store = [&]() {   // rows past the segment and the pad columns as zero
      int r = tr0, c = tc0;
#pragma unroll
      for (int e = 0; e < NS; ++e) {
        if (e < nslot) Wt[r * Fs + c] = keep_if(treg[e], r < nj_ld && c < F);
        r += tdq;
        c += tdr;
        if (c >= F4) {
          c -= F4;
          ++r;
        }
      }
    };

    tile_load(0);
    gw_stage_t(t_in, labels, mode, o, n, heads, hd, ts, lab);
    tile_store();   // (the previous unit's readers passed its last barrier)
    __syncthreads();

    const int ib = i0 + 16 * wave;
    const bool active = ib < n;   // wave-uniform
    const int i = ib + r16;
    const bool iv = i < n;
    float si = 0.f, li = 0.f, mx = -INFINITY, inv = 0.f;
    if (active) {
      if (iv) si = s_in[(size_t)(o + i) * heads + hd];
      li = lab[i];
      // (edge without short circuits and the values selected, not branched on:
      // the LDS reads of the unrolled k-steps are in flight together)
      auto is_edge = [&](int j, float lj) {
        return iv & (j < n) & ((mode == 1) | (i == j) | ((li != 0.f) & (li == lj)));
      };
#pragma unroll 4
      for (int m = 0; m < nm; ++m) {
        const int j = 4 * m + q;
        const float z = lrelu(si + ts[j], alpha);
        mx = is_edge(j, lab[j]) ? fmaxf(mx, z) : mx;
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll 4
      for (int m = 0; m < nm; ++m) {
        const int j = 4 * m + q;
        const float ex = expf(lrelu(si + ts[j], alpha) - mx);
        sum += is_edge(j, lab[j]) ? ex : 0.f;
      }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      inv = iv ? 1.f / sum : 0.f;
      if (q == 0 && iv) {
        rmax[(size_t)(o + i) * heads + hd] = mx;
        rinv[(size_t)(o + i) * heads + hd] = inv;
      }
    }
    floatx4 hv[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) hv[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int jt = 0; jt < ntile; ++jt) {
      if (jt + 1 < ntile) tile_load(kGwT * (jt + 1));
      if (active) {
        const int nk = min(kGwT / 4, nm - (kGwT / 4) * jt);
        for (int mm = 0; mm < nk; ++mm) {
          const int j = kGwT * jt + 4 * mm + q;
          const bool edge = iv & (j < n) & ((mode == 1) | (i == j) | ((li != 0.f) & (li == lab[j])));
          const float ex = expf(lrelu(si + ts[j], alpha) - mx);
          float p = edge ? ex : 0.f;
          p *= inv;
          const float* wr = Wt + (4 * mm + q) * Fs;
#pragma unroll
          for (int ct = 0; ct < 8; ++ct)
            if (ct < nct) hv[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, wr[min(16 * ct + r16, F - 1)], hv[ct], 0, 0, 0);
        }
      }
      __syncthreads();   // tile consumed
      if (jt + 1 < ntile) {
        tile_store();
        __syncthreads();
      }
    }
    if (active) {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        if (ct < nct) {
          const float bv = (bias && 16 * ct + r16 < F) ? bias[16 * ct + r16] : 0.f;
#pragma unroll
          for (int v = 0; v < 4; ++v) hv[ct][v] += bv;
        }
      }
      SGG_GAT_EPILOGUE_STORE(ib)
    }
  }
}

// ---- backward -------------------------------------------------------------------
// d hp of rows [row0, row0 + nv) (global rows) into the 64 x Fs LDS tile Ds
// (zero rows past nv), formed from dy as gat_bwd_kernel does: epilogue 1
// dy ELU'(hp); epilogue 2 (dy - softmax(y) rowsum(dy)) ELU'(hp).  The caller
// barriers afterwards.
__device__ __forceinline__ void gw_stage_dhp(float* Ds, float* rsum, int Fs, int F, int F4, int nv, size_t row0,
                                             int HF, int c0, int epi, const float* __restrict__ hp,
                                             const float* __restrict__ y, const float* __restrict__ dy, int lddy) {
  stage_block(
      kGwT, F4, nv, F,
      [&](int r, int f) {
        const size_t row = row0 + r;
        const float d = dy[row * lddy + c0 + f];
        return epi == 1 ? d * elu_grad(hp[row * HF + c0 + f]) : d;
      },
      [&](int r, int f, float v) { Ds[r * Fs + f] = v; });
  if (epi == 2) {
    __syncthreads();
    {   // row sums of dy: 4 lanes per row
      const int r = threadIdx.x >> 2, part = threadIdx.x & 3;
      float sd = 0.f;
      for (int f = part; f < F; f += 4) sd += Ds[r * Fs + f];
      sd += __shfl_xor(sd, 1);
      sd += __shfl_xor(sd, 2);
      if (part == 0) rsum[r] = sd;
    }
    __syncthreads();
    stage_block(
        nv, F, nv, F,
        [&](int r, int f) {
          const size_t row = row0 + r;
          return (Ds[r * Fs + f] - expf(y[row * F + f]) * rsum[r]) * elu_grad(hp[row * HF + c0 + f]);
        },
        [&](int r, int f, float v) { Ds[r * Fs + f] = v; });
  }
}

// Row units: 64 rows of a (segment, head), 16 per wave in gat_bwd_kernel's C
// layout (lane = column j of a 16-node sub-tile, rows 4 (lane >> 4) + v),
// walking j in tiles of 64 nodes twice: the attention from the saved row
// statistics, datt_ij = dhp_i . Wh_j on the MFMA and dot_i = sum_j att_ij
// datt_ij; then dz and ds_i = sum_j dz_ij.  Writes ds and dot.  Also zeroes
// the gradients of the rows past the last segment.
__global__ void __launch_bounds__(kGatThreads) gat_bwd_wide_rows_kernel(
    const float* __restrict__ Wh, int heads, const float* __restrict__ labels, const int32_t* __restrict__ seg_off,
    int nseg, int nrows, int F, float alpha, int mode, int epi, int max_seg, int nblk, const float* __restrict__ hp,
    const float* __restrict__ y, const float* __restrict__ dy, int lddy, const float* __restrict__ s_in,
    const float* __restrict__ t_in, const float* __restrict__ rmax, const float* __restrict__ rinv,
    float* __restrict__ dot_w, float* __restrict__ ds_w, float* __restrict__ dWh, float* __restrict__ ds_out,
    float* __restrict__ dt_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3, HF = heads * F;
  const int nmax = min(gat_r16(max_seg), kGwMax);
  {  // rows past the last segment: zero gradients
    const size_t r0 = seg_off[nseg], wd = (size_t)heads * (F + 2);
    for (size_t e = r0 * wd + blockIdx.x * kGatThreads + threadIdx.x; e < (size_t)nrows * wd;
         e += (size_t)gridDim.x * kGatThreads) {
      const size_t r = e / wd, c = e - r * wd;
      if (c < (size_t)HF) dWh[r * HF + c] = 0.f;
      else if (c < (size_t)HF + heads) {
        if (ds_out) ds_out[r * heads + c - HF] = 0.f;
      } else if (dt_out) dt_out[r * heads + c - HF - heads] = 0.f;
    }
  }
  float* Dr = reinterpret_cast<float*>(smem);   // kGwT x Fs: d hp of the unit's rows
  float* Wt = Dr + kGwT * Fs;                   // kGwT x Fs: the j tile of Wh
  float* ts = Wt + kGwT * Fs;                   // kGwMax
  float* lab = ts + kGwMax;                     // kGwMax
  float* rsum = lab + kGwMax;                   // kGwT
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const long long units = (long long)nseg * nblk * heads;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const GwUnit w = gw_unit(u, heads, nblk);
    const int o = seg_off[w.g];
    const int n = min(seg_off[w.g + 1] - o, nmax);
    const int i0 = kGwT * w.blk;
    if (i0 >= n) continue;
    const int hd = w.hd, c0 = hd * F;
    const int ntile = (n + kGwT - 1) / kGwT;
    gw_stage_t(t_in, labels, mode, o, n, heads, hd, ts, lab);
    gw_stage_dhp(Dr, rsum, Fs, F, F4, min(kGwT, n - i0), (size_t)(o + i0), HF, c0, epi, hp, y, dy, lddy);
    const int ib = i0 + 16 * wave;
    const bool active = ib < n;   // wave-uniform
    float sv[4], lv[4], mxv[4], inw[4], dot[4], dsr[4];
    bool iv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = ib + 4 * q + v;
      iv[v] = i < n;
      const size_t ih = (size_t)(o + min(i, n - 1)) * heads + hd;
      sv[v] = s_in[ih];
      mxv[v] = rmax[ih];
      inw[v] = iv[v] ? rinv[ih] : 0.f;
      lv[v] = mode == 0 ? labels[o + min(i, n - 1)] : 0.f;
      dot[v] = 0.f;
      dsr[v] = 0.f;
    }
    for (int pass = 0; pass < 2; ++pass) {
      for (int jt = 0; jt < ntile; ++jt) {
        const int jb = kGwT * jt, nj = min(kGwT, n - jb);
        __syncthreads();   // ts / lab / Dr staged; the previous tile consumed
        stage_block(kGwT, F4, nj, F, [&](int r, int f) { return Wh[(size_t)(o + jb + r) * HF + c0 + f]; },
                    [&](int r, int f, float v) { Wt[r * Fs + f] = v; });
        __syncthreads();
        if (!active) continue;
        const float* Da = Dr + (16 * wave + r16) * Fs + q;
        for (int sub = 0; 16 * sub < nj; ++sub) {
          floatx4 da = floatx4{0.f, 0.f, 0.f, 0.f};
          const float* Wb = Wt + (16 * sub + r16) * Fs + q;
          for (int k = 0; k < F4; k += 4) da = __builtin_amdgcn_mfma_f32_16x16x4f32(Da[k], Wb[k], da, 0, 0, 0);
          const int j = jb + 16 * sub + r16;
          const bool jv = j < n;
          const float tj = ts[min(j, n - 1)], lj = lab[min(j, n - 1)];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = ib + 4 * q + v;
            const bool edge = jv && iv[v] && (mode == 1 || i == j || (lv[v] != 0.f && lv[v] == lj));
            const float z = sv[v] + tj;
            const float a = edge ? expf(lrelu(z, alpha) - mxv[v]) * inw[v] : 0.f;
            if (pass == 0) {
              dot[v] = fmaf(a, da[v], dot[v]);
            } else {
              const float de = a * (da[v] - dot[v]);
              dsr[v] += z > 0.f ? de : alpha * de;
            }
          }
        }
      }
      if (pass == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int o2 = 1; o2 < 16; o2 <<= 1) dot[v] += __shfl_xor(dot[v], o2);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
      for (int o2 = 1; o2 < 16; o2 <<= 1) dsr[v] += __shfl_xor(dsr[v], o2);
      if (r16 == 0 && iv[v]) {
        const size_t ih = (size_t)(o + ib + 4 * q + v) * heads + hd;
        dot_w[ih] = dot[v];
        ds_w[ih] = dsr[v];
        if (ds_out) ds_out[ih] = dsr[v];
      }
    }
    __syncthreads();  // LDS reused by the next unit
  }
}

// Column units: 64 columns j of a (segment, head) -- their Wh rows staged
// once -- walking i in tiles of 64 rows, ascending.  Per tile the attention
// and dz are recomputed (wave w: rows 16 w .. 16 w + 15, C layout), dz is
// added to the lane's column sums (dt), the attention tile goes through LDS
// (At, as gat_bwd_kernel's) and wave w adds att^T dhp of its 16 columns to
// its dWh accumulators on the MFMA.  Then dWh_j += ds_j a_src + dt_j a_dst;
// each dWh row and dt are written once.  With the slabs each unit also
// writes its partials of da_src = Wh^T ds, da_dst = Wh^T dt over its nodes
// (pda) and the fp64 column sums of their dhp (pdb); every sum has a fixed
// order.
__global__ void __launch_bounds__(kGatThreads) gat_bwd_wide_cols_kernel(
    const float* __restrict__ Wh, int heads, const float* __restrict__ a_src, const float* __restrict__ a_dst, int lda,
    const float* __restrict__ labels, const int32_t* __restrict__ seg_off, int nseg, int F, float alpha, int mode,
    int epi, int max_seg, int nblk, const float* __restrict__ hp, const float* __restrict__ y,
    const float* __restrict__ dy, int lddy, const float* __restrict__ s_in, const float* __restrict__ t_in,
    const float* __restrict__ rmax, const float* __restrict__ rinv, const float* __restrict__ dot_w,
    const float* __restrict__ ds_w, float* __restrict__ dWh, float* __restrict__ dt_out, float* __restrict__ pda,
    double* __restrict__ pdb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3, HF = heads * F;
  const int nmax = min(gat_r16(max_seg), kGwMax);
  float* Wc = reinterpret_cast<float*>(smem);   // kGwT x Fs: Wh of the unit's columns
  float* Di = Wc + kGwT * Fs;                   // kGwT x Fs: d hp of the i tile
  float* At = Di + kGwT * Fs;                   // kGwT x kGwNa: att of the tile
  float* rs = At + kGwT * kGwNa;                // the i tile's rows: s | max | 1/sum | dot | label
  float* rsum = rs + 5 * kGwT;                  // kGwT
  float* dtw = rsum + kGwT;                     // 4 x kGwT: the waves' column sums
  float* dsl = dtw + kGatWaves * kGwT;          // kGwT: ds of the unit's nodes
  float* dtl = dsl + kGwT;                      // kGwT: dt
  float* al = dtl + kGwT;                       // 2F: the head's a_src | a_dst
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int nct = (F + 15) >> 4;
  const long long units = (long long)nseg * nblk * heads;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const GwUnit w = gw_unit(u, heads, nblk);
    const int o = seg_off[w.g];
    const int n = min(seg_off[w.g + 1] - o, nmax);
    const int j0 = kGwT * w.blk;
    if (j0 >= n) {   // no nodes: zero partials
      for (int c = threadIdx.x; c < 3 * F; c += kGatThreads) {
        if (c < 2 * F) {
          if (pda) pda[(size_t)u * 2 * F + c] = 0.f;
        } else if (pdb) {
          pdb[(size_t)u * F + c - 2 * F] = 0.0;
        }
      }
      continue;
    }
    const int hd = w.hd, c0 = hd * F;
    const int nj = min(kGwT, n - j0);
    const int ntile = (n + kGwT - 1) / kGwT;
    for (int f = threadIdx.x; f < 2 * F; f += kGatThreads)
      al[f] = f < F ? a_src[(size_t)lda * hd + f] : a_dst[(size_t)lda * hd + f - F];
    stage_block(kGwT, F4, nj, F, [&](int r, int f) { return Wh[(size_t)(o + j0 + r) * HF + c0 + f]; },
                [&](int r, int f, float v) { Wc[r * Fs + f] = v; });
    float tj[4], lj[4], dtacc[4];
    bool jv[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int j = j0 + 16 * sub + r16;
      jv[sub] = j < n;
      tj[sub] = t_in[(size_t)(o + min(j, n - 1)) * heads + hd];
      lj[sub] = mode == 0 ? labels[o + min(j, n - 1)] : 0.f;
      dtacc[sub] = 0.f;
    }
    floatx4 acc[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) acc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < ntile; ++it) {
      const int ib = kGwT * it, ni = min(kGwT, n - ib);
      __syncthreads();   // the previous tile's At / Di / rs consumed
      if (threadIdx.x < kGwT) {
        const int r = threadIdx.x;
        const bool rv = r < ni;
        const size_t ih = (size_t)(o + ib + min(r, ni - 1)) * heads + hd;
        rs[r] = s_in[ih];
        rs[kGwT + r] = rmax[ih];
        rs[2 * kGwT + r] = rv ? rinv[ih] : 0.f;
        rs[3 * kGwT + r] = dot_w[ih];
        rs[4 * kGwT + r] = mode == 0 ? labels[o + ib + min(r, ni - 1)] : 0.f;
      }
      gw_stage_dhp(Di, rsum, Fs, F, F4, ni, (size_t)(o + ib), HF, c0, epi, hp, y, dy, lddy);
      __syncthreads();
      if (pdb && it == w.blk) {   // Di holds d hp of the unit's own nodes
        for (int f = threadIdx.x; f < F; f += kGatThreads) {
          double sacc = 0.0;
          for (int r = 0; r < ni; ++r) sacc += (double)Di[r * Fs + f];
          pdb[(size_t)u * F + f] = sacc;
        }
      }
      if (16 * wave < ni) {
        const float* Da = Di + (16 * wave + r16) * Fs + q;
        float sv[4], mxv[4], inw[4], dtv[4], lv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * wave + 4 * q + v;
          sv[v] = rs[r];
          mxv[v] = rs[kGwT + r];
          inw[v] = rs[2 * kGwT + r];
          dtv[v] = rs[3 * kGwT + r];
          lv[v] = rs[4 * kGwT + r];
        }
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          if (16 * sub < nj) {
            floatx4 da = floatx4{0.f, 0.f, 0.f, 0.f};
            const float* Wb = Wc + (16 * sub + r16) * Fs + q;
            for (int k = 0; k < F4; k += 4) da = __builtin_amdgcn_mfma_f32_16x16x4f32(Da[k], Wb[k], da, 0, 0, 0);
            const int j = j0 + 16 * sub + r16;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int r = 16 * wave + 4 * q + v;
              const bool edge = jv[sub] && r < ni && (mode == 1 || ib + r == j || (lv[v] != 0.f && lv[v] == lj[sub]));
              const float z = sv[v] + tj[sub];
              const float a = edge ? expf(lrelu(z, alpha) - mxv[v]) * inw[v] : 0.f;
              const float de = a * (da[v] - dtv[v]);
              dtacc[sub] += z > 0.f ? de : alpha * de;
              At[r * kGwNa + 16 * sub + r16] = a;
            }
          }
        }
      }
      __syncthreads();   // At complete
      if (16 * wave < nj) {   // dWh of columns 16 wave .. + 15 += att^T dhp over the tile's rows
        const int nk = (ni + 3) >> 2;
        for (int m = 0; m < nk; ++m) {
          const float av = At[(4 * m + q) * kGwNa + 16 * wave + r16];
          const float* dr = Di + (4 * m + q) * Fs;
#pragma unroll
          for (int ct = 0; ct < 8; ++ct)
            if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, dr[min(16 * ct + r16, F - 1)], acc[ct], 0, 0, 0);
        }
      }
    }
    // dt: the lanes' column sums joined over the row quarters, then over the waves in order
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      float d = dtacc[sub];
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (q == 0) dtw[wave * kGwT + 16 * sub + r16] = d;
    }
    __syncthreads();
    if (threadIdx.x < kGwT) {
      const int t = threadIdx.x;
      const float d = ((dtw[t] + dtw[kGwT + t]) + dtw[2 * kGwT + t]) + dtw[3 * kGwT + t];
      const bool tv = t < nj;
      dtl[t] = tv ? d : 0.f;
      dsl[t] = tv ? ds_w[(size_t)(o + j0 + t) * heads + hd] : 0.f;
      if (tv && dt_out) dt_out[(size_t)(o + j0 + t) * heads + hd] = d;
    }
    __syncthreads();
    if (pda) {
      for (int c = threadIdx.x; c < 2 * F; c += kGatThreads) {
        const int f = c < F ? c : c - F;
        const float* wv = c < F ? dsl : dtl;
        float pacc = 0.f;
        for (int r = 0; r < nj; ++r) pacc = fmaf(Wc[r * Fs + f], wv[r], pacc);
        pda[(size_t)u * 2 * F + c] = pacc;
      }
    }
    if (16 * wave < nj) {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const int f = 16 * ct + r16;
        if (ct < nct && f < F) {
          const float sf = al[f], df = al[F + f];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int jl = 16 * wave + 4 * q + v;
            if (jl < nj) dWh[(size_t)(o + j0 + jl) * HF + c0 + f] = acc[ct][v] + (dsl[jl] * sf + dtl[jl] * df);
          }
        }
      }
    }
    __syncthreads();  // LDS reused by the next unit
  }
}

static size_t gw_scores_lds(int F) { return sizeof(float) * ((size_t)kGwT * gat_fs(F) + 3 * kGwT + 2 * F) + 16; }
static size_t gw_fwd_lds(int F) { return sizeof(float) * ((size_t)kGwT * gat_fs(F) + 2 * kGwMax) + 16; }
static size_t gw_rows_lds(int F) { return sizeof(float) * ((size_t)2 * kGwT * gat_fs(F) + 2 * kGwMax + kGwT) + 16; }
static size_t gw_cols_lds(int F) {
  return sizeof(float) * ((size_t)2 * kGwT * gat_fs(F) + kGwT * kGwNa + (5 + 1 + kGatWaves + 2) * kGwT + 2 * F) + 16;
}

static int gw_grid(int nseg, int heads, int nblk) {
  const long long w = (long long)nseg * heads * nblk;
  return w < 1 ? 1 : w < 16384 ? (int)w : 16384;
}

// the work buffer's parts
struct GwWork {
  float *s, *t, *rmax, *rinv, *dot, *ds, *pda;
  double* pdb;
};
static GwWork gw_work(float* work, int n, int nseg, int heads, int F, int max_seg) {
  const size_t nh = gw_nh(n, heads), units = (size_t)nseg * gw_blocks(max_seg) * heads;
  GwWork w;
  w.s = work;
  w.t = w.s + nh;
  w.rmax = w.t + nh;
  w.rinv = w.rmax + nh;
  w.dot = w.rinv + nh;
  w.ds = w.dot + nh;
  w.pda = w.ds + nh;
  w.pdb = reinterpret_cast<double*>(w.pda + units * 2 * F);   // (an even float offset: 8-byte aligned)
  return w;
}

}  // namespace sgg

using namespace sgg;

static int gw_args_ok(const char* who, const float* Wh, int heads, const float* as, const float* ad, int lda,
                      const float* labels, const int32_t* off, int nseg, int n, int F, int mode, int epi, int max_seg,
                      const float* work) {
  SGG_CHECK_ARG(Wh && as && ad && off && work, "%s: null pointer", who);
  SGG_CHECK_ARG(((uintptr_t)work & 15) == 0, "%s: work must be 16-byte aligned", who);
  SGG_CHECK_ARG(mode == 0 || mode == 1, "%s: bad mask_mode", who);
  SGG_CHECK_ARG(mode == 1 || labels, "%s: mask_mode 0 needs labels", who);
  SGG_CHECK_ARG(nseg >= 0 && n >= 0, "%s: bad sizes", who);
  SGG_CHECK_ARG(F >= 1 && F <= 128, "%s: F=%d outside [1, 128]", who, F);
  SGG_CHECK_ARG(heads >= 1 && heads <= 64, "%s: heads=%d outside [1, 64]", who, heads);
  SGG_CHECK_ARG(lda >= F, "%s: lda < F", who);
  SGG_CHECK_ARG(epi >= 0 && epi <= 2, "%s: bad epilogue", who);
  SGG_CHECK_ARG(epi != 2 || heads == 1, "%s: the log_softmax epilogue is single-head", who);
  SGG_CHECK_ARG(max_seg >= 1 && max_seg <= SGG_GAT_WIDE_MAX_NODES, "%s: max segment %d outside [1, %d]", who, max_seg,
                SGG_GAT_WIDE_MAX_NODES);
  return 0;
}

extern "C" size_t sgg_gat_wide_work_floats(int n, int nseg, int heads, int F, int max_seg) {
  if (n < 0 || nseg < 0 || heads < 1 || F < 1 || max_seg < 1) return 0;
  return 6 * gw_nh(n, heads) + (size_t)nseg * gw_blocks(max_seg) * heads * 4 * F;
}

extern "C" int sgg_gat_fwd_wide(const float* Wh, int heads, const float* a_src, const float* a_dst, int lda,
                                const float* bias, const float* labels, const int32_t* seg_off, int nseg, int n, int F,
                                float alpha, int mask_mode, int epilogue, int max_seg, float* hp, float* y, int ldy,
                                float* work, void* stream) {
  const char* who = "sgg_gat_fwd_wide";
  if (int rc = gw_args_ok(who, Wh, heads, a_src, a_dst, lda, labels, seg_off, nseg, n, F, mask_mode, epilogue, max_seg,
                          work))
    return rc;
  SGG_CHECK_ARG(y && (epilogue == 0 || hp), "%s: null output", who);
  SGG_CHECK_ARG(ldy >= heads * F, "%s: ldy < heads * F", who);
  SGG_CHECK_ARG(epilogue != 2 || ldy == F, "%s: log_softmax epilogue needs a dense y (ldy == F)", who);
  if (nseg == 0 && n == 0) return 0;   // (rows but no segments: the kernel zeroes the rows)
  const GwWork w = gw_work(work, n, nseg, heads, F, max_seg);
  const int nblk = gw_blocks(max_seg), grid = gw_grid(nseg, heads, nblk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gat_wide_scores_kernel, dim3(grid), dim3(kGatThreads), gw_scores_lds(F), st, Wh, heads, a_src,
                     a_dst, lda, seg_off, nseg, F, max_seg, nblk, w.s, w.t);
  auto k = F <= 32 ? gat_fwd_wide_kernel<8> : F <= 64 ? gat_fwd_wide_kernel<16> : F <= 96 ? gat_fwd_wide_kernel<24>
                                                                                           : gat_fwd_wide_kernel<32>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kGatThreads), gw_fwd_lds(F), st, Wh, heads, bias, labels, seg_off, nseg, n,
                     F, alpha, mask_mode, epilogue, max_seg, nblk, w.s, w.t, w.rmax, w.rinv, hp, y, ldy);
  SGG_RETURN_LAUNCH(who);
}

extern "C" int sgg_gat_bwd_wide(const float* Wh, int heads, const float* a_src, const float* a_dst, int lda,
                                const float* labels, const int32_t* seg_off, int nseg, int n, int F, float alpha,
                                int mask_mode, int epilogue, int max_seg, const float* hp, const float* y,
                                const float* dy, int lddy, float* dWh, float* ds, float* dt, float* da_src,
                                float* da_dst, float* dbias, float* work, void* stream) {
  const char* who = "sgg_gat_bwd_wide";
  if (int rc = gw_args_ok(who, Wh, heads, a_src, a_dst, lda, labels, seg_off, nseg, n, F, mask_mode, epilogue, max_seg,
                          work))
    return rc;
  SGG_CHECK_ARG(dy && dWh, "%s: null pointer", who);
  SGG_CHECK_ARG(epilogue == 0 || hp, "%s: epilogue needs hp", who);
  SGG_CHECK_ARG(epilogue != 2 || y, "%s: log_softmax epilogue needs y", who);
  SGG_CHECK_ARG(lddy >= heads * F, "%s: lddy < heads * F", who);
  SGG_CHECK_ARG((ds != nullptr) == (dt != nullptr), "%s: ds and dt go together", who);
  SGG_CHECK_ARG((da_src != nullptr) == (da_dst != nullptr) && (!dbias || da_src),
                "%s: da_src, da_dst (and dbias) go together", who);
  if (nseg == 0 && n == 0) return 0;
  const GwWork w = gw_work(work, n, nseg, heads, F, max_seg);
  const int nblk = gw_blocks(max_seg), grid = gw_grid(nseg, heads, nblk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gat_bwd_wide_rows_kernel, dim3(grid), dim3(kGatThreads), gw_rows_lds(F), st, Wh, heads, labels,
                     seg_off, nseg, n, F, alpha, mask_mode, epilogue, max_seg, nblk, hp, y, dy, lddy, w.s, w.t, w.rmax,
                     w.rinv, w.dot, w.ds, dWh, ds, dt);
  hipLaunchKernelGGL(gat_bwd_wide_cols_kernel, dim3(grid), dim3(kGatThreads), gw_cols_lds(F), st, Wh, heads, a_src,
                     a_dst, lda, labels, seg_off, nseg, F, alpha, mask_mode, epilogue, max_seg, nblk, hp, y, dy, lddy,
                     w.s, w.t, w.rmax, w.rinv, w.dot, w.ds, dWh, dt, da_src ? w.pda : nullptr,
                     dbias ? w.pdb : nullptr);
  // (a grid smaller than the units strides over them, so every slab row is written)
  if (da_src) gat_param_reduce(w.pda, dbias ? w.pdb : nullptr, nseg * nblk, heads, F, da_src, da_dst, dbias, st);
  SGG_RETURN_LAUNCH(who);
}
