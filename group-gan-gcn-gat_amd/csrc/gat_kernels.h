// The attention kernels of gat.hip, included twice (no include guard): with
// SGG_GAT_DROP 0 this text is gat_fwd_kernel / gat_bwd_kernel, with
// SGG_GAT_DROP 1 gat_fwd_drop_kernel / gat_bwd_drop_kernel, which take the
// dropout arguments (DropArgs, dropout_common.h) as one more parameter and
// apply the mask to the normalised attention.
#undef SGG_GAT_FWD_KERNEL
#undef SGG_GAT_BWD_KERNEL
#undef SGG_GAT_DROP_PARAM
#if SGG_GAT_DROP
#define SGG_GAT_FWD_KERNEL gat_fwd_drop_kernel
#define SGG_GAT_BWD_KERNEL gat_bwd_drop_kernel
#define SGG_GAT_DROP_PARAM , const DropArgs drop
#else
#define SGG_GAT_FWD_KERNEL gat_fwd_kernel
#define SGG_GAT_BWD_KERNEL gat_bwd_kernel
#define SGG_GAT_DROP_PARAM
#endif

template <int NM>   // 4-node k-steps held per lane: segments of <= 4 NM nodes
__global__ void __launch_bounds__(kGatThreads) SGG_GAT_FWD_KERNEL(
    const float* __restrict__ Wh, int heads, const float* __restrict__ a_src, const float* __restrict__ a_dst, int lda,
    const float* __restrict__ bias, const float* __restrict__ labels, const int32_t* __restrict__ seg_off, int nseg,
    int nrows, int F, float alpha, int mode, int epi, int max_seg, float* __restrict__ hp, float* __restrict__ y,
    int ldy SGG_GAT_DROP_PARAM) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3;
  const int nmax = gat_r16(max_seg);
  const int HF = heads * F;
  gat_zero_pad_rows(seg_off[nseg], nrows, HF, y, ldy, epi ? hp : nullptr);
  float* Ws = reinterpret_cast<float*>(smem);   // nmax x Fs
  float* ss = Ws + nmax * Fs;                   // nmax
  float* ts = ss + nmax;                        // nmax
  float* lab = ts + nmax;                       // nmax
  float* al = lab + nmax;                       // 2F: the head's a_src | a_dst
  for (int gh = blockIdx.x; gh < nseg * heads; gh += gridDim.x) {
    const int g = gh / heads, hd = gh - g * heads;
    const int o = seg_off[g];
    // (a segment larger than the caller's max_seg would overrun the LDS plan:
    // clamped, memory-safe; the host builds max_seg from the same offsets)
    const int n = min(seg_off[g + 1] - o, nmax);
    if (n <= 0) continue;
    const int c0 = hd * F;
    const int nr = gat_r16(n);
    stage_block(nr, F4, n, F, [&](int r, int f) { return Wh[(size_t)(o + r) * HF + c0 + f]; },
                [&](int r, int f, float v) { Ws[r * Fs + f] = v; });
    for (int f = threadIdx.x; f < 2 * F; f += kGatThreads)
      al[f] = f < F ? a_src[(size_t)lda * hd + f] : a_dst[(size_t)lda * hd + f - F];
    __syncthreads();
    gat_scores(Ws, Fs, al, al + F, F, labels, mode, o, n, nr, ss, ts, lab);
    __syncthreads();
#if SGG_GAT_DROP
    gat_attend<NM, true>(Ws, Fs, ss, ts, lab, o, n, nr, F, HF, c0, alpha, mode, epi, bias, hp, y, ldy,
                         drop_key(drop, hd));
#else
    gat_attend<NM>(Ws, Fs, ss, ts, lab, o, n, nr, F, HF, c0, alpha, mode, epi, bias, hp, y, ldy);
#endif
    __syncthreads();  // LDS reused by the next segment
  }
}

// Backward.  Per row block (in the C layout: lane = column j, rows 4 (lane >>
// 4) + v): the attention recomputed, datt = dhp @ Wh^T on MFMA, the softmax
// and LeakyReLU backward to dz, its row sums (ds) and per-block column sums
// (dt, summed over the blocks in order afterwards); the attention goes to LDS
// for dWh = att^T @ dhp (MFMA over the rows) + ds a_src + dt a_dst.
// With the slabs (sgg_gat_bwd_ex) each (segment, head) also writes its
// partials of the parameter gradients: da_src = Wh^T ds, da_dst = Wh^T dt
// (pda, 2F floats) and the bias gradient's column sums of dhp (pdb, F doubles:
// a near-cancelling sum, the next layer's instance norm removes each
// feature's scene mean); gat_param_reduce_kernel sums them in a fixed order.
// With attention dropout (m the scaled mask the forward applied to att):
// datt = m (dhp Wh^T), the softmax backward runs on the undropped att, and the
// tile that goes to LDS for dWh is att m.  A lane's NJT x 4 mask decisions are
// one 32-bit word (bit 4 jt + v), generated once per row block: rows o + 16 rb
// + 4 q + v of the node array share one Philox call per column when the
// segment starts on a multiple of 4 rows, and span two otherwise.
template <int NJT>  // 16-node column tiles: segments of <= 16 NJT nodes
__global__ void __launch_bounds__(kGatThreads) SGG_GAT_BWD_KERNEL(
    const float* __restrict__ Wh, int heads, const float* __restrict__ a_src, const float* __restrict__ a_dst, int lda,
    const float* __restrict__ labels, const int32_t* __restrict__ seg_off, int nseg, int nrows, int F, float alpha,
    int mode, int epi, int max_seg, const float* __restrict__ hp, const float* __restrict__ y,
    const float* __restrict__ dy, int lddy, float* __restrict__ dWh, float* __restrict__ ds_out,
    float* __restrict__ dt_out, float* __restrict__ pda, double* __restrict__ pdb SGG_GAT_DROP_PARAM) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int gfirst = min((int)blockIdx.x / heads, nseg);
  const int tot = seg_off[nseg], ofirst = seg_off[gfirst], efirst = seg_off[min(gfirst + 1, nseg)];
  {  // rows past the last segment: zero gradients
    const size_t r0 = tot, w = (size_t)heads * (F + 2);
    for (size_t e = r0 * w + blockIdx.x * kGatThreads + threadIdx.x; e < (size_t)nrows * w;
         e += (size_t)gridDim.x * kGatThreads) {
      const size_t r = e / w, c = e - r * w;
      if (c < (size_t)heads * F) dWh[r * heads * F + c] = 0.f;
      else if (!ds_out) continue;
      else if (c < (size_t)heads * (F + 1)) ds_out[r * heads + c - (size_t)heads * F] = 0.f;
      else dt_out[r * heads + c - (size_t)heads * (F + 1)] = 0.f;
    }
  }
  const int Fs = gat_fs(F), F4 = (F + 3) & ~3;
  const int nmax = gat_r16(max_seg), Na = nmax + 4;
  float* Ws = reinterpret_cast<float*>(smem);  // nmax x Fs
  float* Ds = Ws + nmax * Fs;                  // nmax x Fs  (d hp)
  float* At = Ds + nmax * Fs;                  // nmax x Na  (att)
  float* ss = At + nmax * Na;
  float* ts = ss + nmax;
  float* lab = ts + nmax;
  float* dss = lab + nmax;
  float* dts = dss + nmax;
  float* rsum = dts + nmax;                    // epilogue 2: row sums of dy
  float* dtp = rsum + nmax;                    // (nmax / 16) x nmax column partials of dz
  float* al = dtp + (nmax / 16) * nmax;        // 2F: the head's a_src | a_dst
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int HF = heads * F;
  const int nct = (F + 15) >> 4;
  for (int gh = blockIdx.x; gh < nseg * heads; gh += gridDim.x) {
    const int g = gh / heads, hd = gh - g * heads;
    const int o = gh == (int)blockIdx.x ? ofirst : seg_off[g];
    const int n = min((gh == (int)blockIdx.x ? efirst : seg_off[g + 1]) - o, nmax);   // (LDS plan bound)
    if (n <= 0) {
      for (int c = threadIdx.x; c < 3 * F; c += kGatThreads) {
        if (c < 2 * F) {
          if (pda) pda[(size_t)gh * 2 * F + c] = 0.f;
        } else if (pdb) {
          pdb[(size_t)gh * F + c - 2 * F] = 0.0;
        }
      }
      continue;
    }
    const float* as = al;
    const float* ad = al + F;
    const int c0 = hd * F;
    const int nr = gat_r16(n), nrb = nr >> 4;
    for (int f = threadIdx.x; f < 2 * F; f += kGatThreads)
      al[f] = f < F ? a_src[(size_t)lda * hd + f] : a_dst[(size_t)lda * hd + f - F];
    stage_block(nr, F4, n, F, [&](int r, int f) { return Wh[(size_t)(o + r) * HF + c0 + f]; },
                [&](int r, int f, float v) { Ws[r * Fs + f] = v; });
    stage_block(
        nr, F4, n, F,
        [&](int r, int f) {
          const size_t row = (size_t)(o + r);
          const float d = dy[row * lddy + c0 + f];
          return epi == 1 ? d * elu_grad(hp[row * HF + c0 + f]) : d;
        },
        [&](int r, int f, float v) { Ds[r * Fs + f] = v; });
    __syncthreads();
    gat_scores(Ws, Fs, as, ad, F, labels, mode, o, n, nr, ss, ts, lab, Ds, rsum);
    __syncthreads();
    if (epi == 2) {   // d hp = (dy - softmax(y) sum(dy)) * ELU'(hp)
      stage_block(
          n, F, n, F,
          [&](int r, int f) {
            const size_t row = (size_t)(o + r);
            return (Ds[r * Fs + f] - expf(y[row * F + f]) * rsum[r]) * elu_grad(hp[row * HF + c0 + f]);
          },
          [&](int r, int f, float v) { Ds[r * Fs + f] = v; });
      __syncthreads();
    }
    for (int rb = wave; rb < nrb; rb += kGatWaves) {
      float sv[4], lv[4];
      bool iv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 16 * rb + 4 * q + v;
        iv[v] = i < n;
        sv[v] = ss[i];
        lv[v] = lab[i];
      }
      float tj[NJT], att[NJT][4];
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) {
        const int j = 16 * jt + r16;
        const bool jv = jt < nrb && j < n;
        tj[jt] = jt < nrb ? ts[j] : 0.f;
        const float lj = jt < nrb ? lab[j] : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = 16 * rb + 4 * q + v;
          const bool edge = jv && iv[v] && (mode == 1 || i == j || (lv[v] != 0.f && lv[v] == lj));
          att[jt][v] = edge ? lrelu(sv[v] + tj[jt], alpha) : -INFINITY;
          mx[v] = fmaxf(mx[v], att[jt][v]);
        }
      }
      float inv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) mx[v] = fmaxf(mx[v], __shfl_xor(mx[v], o2));
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) {
          const float e = att[jt][v] == -INFINITY ? 0.f : expf(att[jt][v] - mx[v]);
          att[jt][v] = e;
          sum += e;
        }
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) sum += __shfl_xor(sum, o2);
        inv[v] = iv[v] ? 1.f / sum : 0.f;
      }
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int v = 0; v < 4; ++v) att[jt][v] *= inv[v];
#if SGG_GAT_DROP
      uint32_t keep = 0;   // bit 4 jt + v: element (row 4 q + v, column tile jt) is kept
      const DropKey dk = drop_key(drop, hd);
      {
        const uint32_t r0 = (uint32_t)(o + 16 * rb + 4 * q), sh = r0 & 3;   // (sh: uniform over the workgroup)
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) {
          if (jt < nrb) {
            const uint32_t col = 16 * jt + r16;
            const Philox4 x0 = drop_words(dk, r0 >> 2, col);
            uint32_t w[4] = {x0.w[0], x0.w[1], x0.w[2], x0.w[3]};
            if (sh) {
              const Philox4 x1 = drop_words(dk, (r0 >> 2) + 1, col);
              if (sh == 1) w[0] = x0.w[1], w[1] = x0.w[2], w[2] = x0.w[3], w[3] = x1.w[0];
              else if (sh == 2) w[0] = x0.w[2], w[1] = x0.w[3], w[2] = x1.w[0], w[3] = x1.w[1];
              else w[0] = x0.w[3], w[1] = x1.w[0], w[2] = x1.w[1], w[3] = x1.w[2];
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) keep |= (uint32_t)(w[v] >= dk.thr) << (4 * jt + v);
          }
        }
      }
#endif
      // datt_ij = dhp_i . Wh_j
      floatx4 da[NJT];
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) da[jt] = floatx4{0.f, 0.f, 0.f, 0.f};
      const float* Dr = Ds + (16 * rb + r16) * Fs + q;
      for (int k = 0; k < F4; k += 4) {
        const float av = Dr[k];
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt)
          if (jt < nrb) da[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Ws[(16 * jt + r16) * Fs + k + q], da[jt], 0, 0, 0);
      }
#if SGG_GAT_DROP   // datt_ij = m_ij (dhp_i . Wh_j)
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int v = 0; v < 4; ++v) da[jt][v] = (keep >> (4 * jt + v)) & 1 ? da[jt][v] * dk.scale : 0.f;
#endif
      float dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int v = 0; v < 4; ++v) dot[v] = fmaf(att[jt][v], da[jt][v], dot[v]);
      float dsr[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) dot[v] += __shfl_xor(dot[v], o2);
        dsr[v] = 0.f;
      }
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) {
        if (jt < nrb) {
          float cp = 0.f;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float de = att[jt][v] * (da[jt][v] - dot[v]);
            const float dz = (sv[v] + tj[jt]) > 0.f ? de : alpha * de;
            dsr[v] += dz;
            cp += dz;
#if SGG_GAT_DROP
            At[(16 * rb + 4 * q + v) * Na + 16 * jt + r16] = (keep >> (4 * jt + v)) & 1 ? att[jt][v] * dk.scale : 0.f;
#else
            At[(16 * rb + 4 * q + v) * Na + 16 * jt + r16] = att[jt][v];
#endif
          }
          cp += __shfl_xor(cp, 16);
          cp += __shfl_xor(cp, 32);
          if (q == 0) dtp[rb * nmax + 16 * jt + r16] = cp;
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) dsr[v] += __shfl_xor(dsr[v], o2);
        if (r16 == 0) dss[16 * rb + 4 * q + v] = dsr[v];
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nr; j += kGatThreads) {
      float acc = 0.f;
      for (int rb = 0; rb < nrb; ++rb) acc += dtp[rb * nmax + j];
      dts[j] = acc;
      if (j < n && ds_out) {
        ds_out[(size_t)(o + j) * heads + hd] = dss[j];
        dt_out[(size_t)(o + j) * heads + hd] = acc;
      }
    }
    __syncthreads();
    // parameter-gradient partials of this (segment, head): LDS reads only
    for (int c = threadIdx.x; c < 3 * F; c += kGatThreads) {
      if (c < 2 * F) {
        if (pda) {
          const int f = c < F ? c : c - F;
          const float* wv = c < F ? dss : dts;
          float acc = 0.f;
          for (int i = 0; i < n; ++i) acc = fmaf(Ws[i * Fs + f], wv[i], acc);
          pda[(size_t)gh * 2 * F + c] = acc;
        }
      } else if (pdb) {
        const int f = c - 2 * F;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (double)Ds[i * Fs + f];
        pdb[(size_t)gh * F + f] = acc;
      }
    }
    // dWh_j = sum_i att_ij dhp_i + ds_j a_src + dt_j a_dst
    for (int jb = wave; jb < nrb; jb += kGatWaves) {
      for (int ct = 0; ct < nct; ++ct) {
        const int fb = min(16 * ct + r16, F - 1);
        floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < nr; m += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(At[(m + q) * Na + 16 * jb + r16], Ds[(m + q) * Fs + fb], acc, 0,
                                                     0, 0);
        const int f = 16 * ct + r16;
        if (f < F) {
          const float sf = as[f], df = ad[f];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int j = 16 * jb + 4 * q + v;
            if (j < n) dWh[(size_t)(o + j) * HF + c0 + f] = acc[v] + (dss[j] * sf + dts[j] * df);
          }
        }
      }
    }
    __syncthreads();  // LDS reused by the next segment
  }
}
