// Generic LSTM sequence kernels: every hidden size 1 <= H <= 128 the four-wave
// family (lstm_mw.hip) is not built for.  fp32 on v_mfma_f32_16x16x4_f32, 16
// peds per workgroup, the true H a runtime argument, the kernels templated on
// the padded tile count HT = ceil(H / 16) (1..8).  DESIGN.md 4h.
//
// Layout.  One workgroup = 16 peds = HT waves.  Wave w owns the hidden units
// [16 w, 16 w + 16) with all four gates: its rows of W_hh (forward) or its
// rows of W_hh^T (backward) stay in registers as MFMA A operands for the whole
// sequence (16 HT floats per lane: 128 VGPRs at H = 128), and the B operand --
// h_{t-1} (forward) or the gate gradients dG_t (backward), k x 16 peds -- is
// exchanged through LDS once per step.  An accumulator tile is D[unit][ped]:
// lane (c16 = lane & 15, kq = lane >> 4) holds units 16 w + 4 kq + r, r < 4,
// of ped c16, and the four gates of a (unit, ped) pair land in the same lane,
// so the cell update and its backward are lane-local.
//
// Padding.  Units, rows and k-steps past H are zero operands: a padded unit
// has zero gates, so i = f = o = 1/2, g = 0, c = 0, h = 0 exactly, and its
// gate gradients are exactly zero.  Every access to a caller's B x H (or
// 4H x H) buffer is masked by unit < H and ped < B; only the saved states
// (act_all, c_all) are padded, and they are the family's own tile-native
// layout (lstm_gen_state_floats).
//
// The input term A r + bias is one more MFMA k-step: A operand [A[:,0] |
// A[:,1] | bias | 0], B operand [r0; r1; 1; 0].
//
// Weight gradients are not formed here: the backward runs the recurrence only
// and writes each step's gate gradients to a stacked (T x B x 4H) buffer; the
// caller forms dW_hh = dG^T h_prev, dA = dG^T r and the bias sums with
// sgg_xtw_partial / sgg_grad_finish (fixed order, no atomics) -- the form of
// dec_step.hip.
#include "sgg_common.h"

namespace sgg {

constexpr int kGenPeds = 16;
constexpr float kGenNegLog2e = -1.4426950408889634f;

// v_exp_f32 / v_rcp_f32 forms, as the other LSTM kernels (lstm_mw.hip)
__device__ __forceinline__ float gen_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * kGenNegLog2e));
}
__device__ __forceinline__ float gen_tanh(float x) {
  return fmaf(2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * (2.f * kGenNegLog2e))), -1.f);
}

struct GenFwd {
  const float *rel, *A, *Whh, *bias, *h0, *c0, *Wp, *bp;
  int T, B, H;
  float *h_all, *c_all, *act_all, *rel_out;
};

struct GenBwd {
  const float *A, *Whh, *Wp, *c_all, *act_all, *dh_last, *dout;
  int T, B, H;
  float *dG, *dh0, *drel_in, *drel_tot;
};

// saved states, tile-native: act_all[t][blk][w][gate][lane][r], c_all[t][blk][w][lane][r]
// (c_all index 0 = the initial cells, t + 1 = the cells after step t)
__device__ __forceinline__ size_t gen_act_off(int t, int nblk, int blk, int HT, int w, int gate, int lane) {
  return ((((size_t)t * nblk + blk) * HT + w) * 4 + gate) * 256 + (size_t)lane * 4;
}
__device__ __forceinline__ size_t gen_c_off(int t, int nblk, int blk, int HT, int w, int lane) {
  return (((size_t)t * nblk + blk) * HT + w) * 256 + (size_t)lane * 4;
}

template <int HT, bool DEC, bool SAVE>
__global__ void __launch_bounds__(64 * HT) lstm_gen_fwd_kernel(GenFwd p) {
  constexpr int HP = 16 * HT;
  __shared__ float hs[2][HP * kGenPeds];           // h_{t-1}: [unit][ped], double-buffered
  __shared__ float rp[2][HT][kGenPeds][2];         // decoder: the waves' partial Wp h
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c16 = lane & 15, kq = lane >> 4;
  const int T = p.T, B = p.B, H = p.H;
  const int blk = blockIdx.x, nblk = gridDim.x;
  const int ped = blk * kGenPeds + c16;
  const bool pok = ped < B;
  const size_t pc = (size_t)(pok ? ped : B - 1);   // clamped: a padded column computes on a copy of the last ped

  // A operands: lane (m = c16, k = kq) of k-step s holds W_hh[gate H + 16 w + c16][4 s + kq]
  float wreg[4][4 * HT], aext[4];
  {
    const int unit = 16 * w + c16;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int s = 0; s < 4 * HT; ++s) {
        const int k = 4 * s + kq;
        wreg[g][s] = (unit < H && k < H) ? p.Whh[((size_t)g * H + unit) * H + k] : 0.f;
      }
      float v = 0.f;
      if (unit < H) {
        const size_t row = (size_t)g * H + unit;
        v = kq == 0 ? p.A[row * 2] : kq == 1 ? p.A[row * 2 + 1] : kq == 2 ? p.bias[row] : 0.f;
      }
      aext[g] = v;
    }
  }
  // the lane's cells: units ju + r of ped c16
  const int ju = 16 * w + 4 * kq;
  float c[4], wp0[4], wp1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = ju + r < H;
    c[r] = (p.c0 && ok) ? p.c0[pc * H + ju + r] : 0.f;
    const float h = (p.h0 && ok) ? p.h0[pc * H + ju + r] : 0.f;
    hs[0][(ju + r) * kGenPeds + c16] = h;
    if (SAVE && ok && pok) p.h_all[(size_t)ped * H + ju + r] = h;
    wp0[r] = (DEC && ok) ? p.Wp[ju + r] : 0.f;
    wp1[r] = (DEC && ok) ? p.Wp[H + ju + r] : 0.f;
  }
  if (SAVE) *reinterpret_cast<float4*>(p.c_all + gen_c_off(0, nblk, blk, HT, w, lane)) = make_float4(c[0], c[1], c[2], c[3]);
  float bp0 = 0.f, bp1 = 0.f;
  if (DEC) {
    bp0 = p.bp[0];
    bp1 = p.bp[1];
  }
  // B operand of the input k-step: lane (k = kq, n = c16) holds [r0; r1; 1; 0][kq] of ped c16
  float rext = kq < 2 ? p.rel[pc * 2 + kq] : kq == 2 ? 1.f : 0.f;
  lds_barrier();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    float rnext = 0.f;
    if (!DEC && t + 1 < T && kq < 2) rnext = p.rel[((size_t)(t + 1) * B + pc) * 2 + kq];
    floatx4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(aext[g], rext, floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4 * HT; ++s) {
      const float hb = hs[cur][(4 * s + kq) * kGenPeds + c16];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[g][s], hb, acc[g], 0, 0, 0);
    }
    // gates (PyTorch order i, f, g, o), cell update
    float gi[4], gf[4], gg[4], go[4], h[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gi[r] = gen_sigmoid(acc[0][r]);
      gf[r] = gen_sigmoid(acc[1][r]);
      gg[r] = gen_tanh(acc[2][r]);
      go[r] = gen_sigmoid(acc[3][r]);
      c[r] = fmaf(gf[r], c[r], gi[r] * gg[r]);
      h[r] = go[r] * gen_tanh(c[r]);
      hs[cur ^ 1][(ju + r) * kGenPeds + c16] = h[r];
    }
    if (SAVE || t == T - 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (pok && ju + r < H) p.h_all[((size_t)(t + 1) * B + ped) * H + ju + r] = h[r];
    }
    if (SAVE) {
      *reinterpret_cast<float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 0, lane)) = make_float4(gi[0], gi[1], gi[2], gi[3]);
      *reinterpret_cast<float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 1, lane)) = make_float4(gf[0], gf[1], gf[2], gf[3]);
      *reinterpret_cast<float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 2, lane)) = make_float4(gg[0], gg[1], gg[2], gg[3]);
      *reinterpret_cast<float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 3, lane)) = make_float4(go[0], go[1], go[2], go[3]);
      *reinterpret_cast<float4*>(p.c_all + gen_c_off(t + 1, nblk, blk, HT, w, lane)) = make_float4(c[0], c[1], c[2], c[3]);
    }
    if (DEC) {
      // hidden2pos: the wave's 16 units, summed over r then over kq (fixed order)
      float q0 = 0.f, q1 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        q0 = fmaf(wp0[r], h[r], q0);
        q1 = fmaf(wp1[r], h[r], q1);
      }
      q0 += __shfl_xor(q0, 16);
      q1 += __shfl_xor(q1, 16);
      q0 += __shfl_xor(q0, 32);
      q1 += __shfl_xor(q1, 32);
      if (kq == 0) {
        rp[cur][w][c16][0] = q0;
        rp[cur][w][c16][1] = q1;
      }
    }
    lds_barrier();
    if (DEC) {
      float r0 = bp0, r1 = bp1;   // the waves' partials in wave order
#pragma unroll
      for (int v = 0; v < HT; ++v) {
        r0 += rp[cur][v][c16][0];
        r1 += rp[cur][v][c16][1];
      }
      if (w == 0 && kq == 0 && pok) {
        p.rel_out[((size_t)t * B + ped) * 2] = r0;
        p.rel_out[((size_t)t * B + ped) * 2 + 1] = r1;
      }
      rext = kq == 0 ? r0 : kq == 1 ? r1 : kq == 2 ? 1.f : 0.f;
    } else {
      rext = kq < 2 ? rnext : rext;
    }
  }
  if (!SAVE && p.c_all)   // the final cells, at their place of the saved layout
    *reinterpret_cast<float4*>(p.c_all + gen_c_off(T, nblk, blk, HT, w, lane)) = make_float4(c[0], c[1], c[2], c[3]);
}

// BPTT, the recurrence only.  Step t (T-1 .. 0), then the epilogue "t = -1":
//   top:     dh_rec = W_hh^T dG_{t+1} and the waves' partials of drin(t+1) = A^T dG_{t+1} from the LDS image of
//            dG_{t+1} (the same B operands feed both), partials to LDS;                           barrier 1
//   then:    drin(t+1) in wave order -> drel_in[t+1]; decoder: drel_tot[t] = dout[t] + drin(t+1),
//            dh = dh_rec + Wp^T drel_tot[t]; encoder: dh = dh_rec (+ dh_last at t = T-1);
//            the cell backward, dG_t to LDS and to the stacked buffer;                            barrier 2
template <int HT, bool DEC>
__global__ void __launch_bounds__(64 * HT) lstm_gen_bwd_kernel(GenBwd p) {
  constexpr int HP = 16 * HT;
  constexpr int KS = 4 * HT;                         // k-steps per gate block
  __shared__ float dgs[4 * HP * kGenPeds];          // dG_t: [gate HP + unit][ped]
  __shared__ float dp[HT][kGenPeds][2];             // the waves' partial A^T dG
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c16 = lane & 15, kq = lane >> 4;
  const int T = p.T, B = p.B, H = p.H;
  const int blk = blockIdx.x, nblk = gridDim.x;
  const int ped = blk * kGenPeds + c16;
  const bool pok = ped < B;
  const size_t pc = (size_t)(pok ? ped : B - 1);

  // A operands: W_hh^T, lane (m = c16, k = kq) of gate g, k-step s holds W_hh[g H + 4 s + kq][16 w + c16];
  // at[i]: the wave's slice (k-steps 16 w + i of the 16 HT) of A^T, rows m = 0, 1
  float wt[4][KS], at[16];
  {
    const int unit = 16 * w + c16;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int jj = 4 * s + kq;
        wt[g][s] = (unit < H && jj < H) ? p.Whh[((size_t)g * H + jj) * H + unit] : 0.f;
      }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = 16 * w + i, g = q / KS, jj = 4 * (q - g * KS) + kq;
      at[i] = (c16 < 2 && jj < H) ? p.A[((size_t)g * H + jj) * 2 + c16] : 0.f;
    }
  }
  const int ju = 16 * w + 4 * kq;
  float wp0[4], wp1[4], dcn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = ju + r < H;
    wp0[r] = (DEC && ok) ? p.Wp[ju + r] : 0.f;
    wp1[r] = (DEC && ok) ? p.Wp[H + ju + r] : 0.f;
  }
  float4 ct = *reinterpret_cast<const float4*>(p.c_all + gen_c_off(T, nblk, blk, HT, w, lane));   // c after step t

  for (int t = T - 1; t >= -1; --t) {
    const bool have = t < T - 1;
    // this step's saved states and output gradients: issued before the MFMA pass that hides them
    float4 ai = {}, af = {}, ag = {}, ao = {}, cp = {};
    float d0 = 0.f, d1 = 0.f, dl[4] = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0) {
      ai = *reinterpret_cast<const float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 0, lane));
      af = *reinterpret_cast<const float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 1, lane));
      ag = *reinterpret_cast<const float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 2, lane));
      ao = *reinterpret_cast<const float4*>(p.act_all + gen_act_off(t, nblk, blk, HT, w, 3, lane));
      cp = *reinterpret_cast<const float4*>(p.c_all + gen_c_off(t, nblk, blk, HT, w, lane));
      if (DEC) {
        d0 = keep_if(p.dout[((size_t)t * B + pc) * 2], pok);
        d1 = keep_if(p.dout[((size_t)t * B + pc) * 2 + 1], pok);
      } else if (t == T - 1 && p.dh_last) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pok && ju + r < H) dl[r] = p.dh_last[pc * H + ju + r];
      }
    }
    floatx4 acc[4], accr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (have) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float b = dgs[(g * HP + 4 * s + kq) * kGenPeds + c16];
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[g][s], b, acc[g], 0, 0, 0);
          const int q = g * KS + s;
          if ((q >> 4) == w) accr = __builtin_amdgcn_mfma_f32_16x16x4f32(at[q & 15], b, accr, 0, 0, 0);
        }
      if (kq == 0) {   // rows m = 0, 1 of the tile: lanes kq = 0, r = 0, 1
        dp[w][c16][0] = accr[0];
        dp[w][c16][1] = accr[1];
      }
    }
    lds_barrier();
    float q0 = 0.f, q1 = 0.f;
    if (have) {
#pragma unroll
      for (int v = 0; v < HT; ++v) {
        q0 += dp[v][c16][0];
        q1 += dp[v][c16][1];
      }
      if (w == 0 && kq == 0 && pok) {
        p.drel_in[((size_t)(t + 1) * B + ped) * 2] = q0;
        p.drel_in[((size_t)(t + 1) * B + ped) * 2 + 1] = q1;
      }
    }
    float dh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[r] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    if (t < 0) {
      if (p.dh0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pok && ju + r < H) p.dh0[(size_t)ped * H + ju + r] = dh[r];
      }
      break;
    }
    if (DEC) {
      d0 += q0;
      d1 += q1;
      if (w == 0 && kq == 0 && pok) {
        p.drel_tot[((size_t)t * B + ped) * 2] = d0;
        p.drel_tot[((size_t)t * B + ped) * 2 + 1] = d1;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[r] += fmaf(wp0[r], d0, wp1[r] * d1);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[r] += dl[r];
    }
    const float vi[4] = {ai.x, ai.y, ai.z, ai.w}, vf[4] = {af.x, af.y, af.z, af.w};
    const float vg[4] = {ag.x, ag.y, ag.z, ag.w}, vo[4] = {ao.x, ao.y, ao.z, ao.w};
    const float vc[4] = {ct.x, ct.y, ct.z, ct.w}, vp[4] = {cp.x, cp.y, cp.z, cp.w};
    float dg[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float tc = gen_tanh(vc[r]);
      const float dc = fmaf(dh[r] * vo[r], 1.f - tc * tc, dcn[r]);
      dg[0][r] = dc * vg[r] * vi[r] * (1.f - vi[r]);
      dg[1][r] = dc * vp[r] * vf[r] * (1.f - vf[r]);
      dg[2][r] = dc * vi[r] * (1.f - vg[r] * vg[r]);
      dg[3][r] = dh[r] * tc * vo[r] * (1.f - vo[r]);
      dcn[r] = dc * vf[r];
    }
    ct = cp;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dgs[(g * HP + ju + r) * kGenPeds + c16] = dg[g][r];
        if (p.dG && pok && ju + r < H) p.dG[((size_t)t * B + ped) * 4 * H + (size_t)g * H + ju + r] = dg[g][r];
      }
    lds_barrier();
  }
}

template <int HT>
static int gen_launch_fwd(const GenFwd& a, bool dec, bool save, hipStream_t st) {
  const dim3 grid((a.B + kGenPeds - 1) / kGenPeds), block(64 * HT);
  if (dec) {
    if (save) hipLaunchKernelGGL((lstm_gen_fwd_kernel<HT, true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((lstm_gen_fwd_kernel<HT, true, false>), grid, block, 0, st, a);
  } else {
    if (save) hipLaunchKernelGGL((lstm_gen_fwd_kernel<HT, false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((lstm_gen_fwd_kernel<HT, false, false>), grid, block, 0, st, a);
  }
  SGG_RETURN_LAUNCH("sgg_lstm_fwd");
}

template <int HT>
static int gen_launch_bwd(const GenBwd& a, bool dec, hipStream_t st) {
  const dim3 grid((a.B + kGenPeds - 1) / kGenPeds), block(64 * HT);
  if (dec) hipLaunchKernelGGL((lstm_gen_bwd_kernel<HT, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((lstm_gen_bwd_kernel<HT, false>), grid, block, 0, st, a);
  SGG_RETURN_LAUNCH("sgg_lstm_bwd");
}

bool lstm_gen_ok(int H) { return H >= 1 && H <= 128 && !lstm_mw_ok(H); }

int lstm_gen_tiles(int H) { return (H + 15) / 16; }

long long lstm_gen_state_floats(int T, int B, int H, int which) {
  const long long padded = (long long)(B + kGenPeds - 1) / kGenPeds * kGenPeds, hp = 16ll * lstm_gen_tiles(H);
  return which == 0 ? (long long)T * padded * 4 * hp : (long long)(T + 1) * padded * hp;
}

int lstm_gen_fwd(const float* rel, const float* A, const float* Whh, const float* bias, const float* h0,
                 const float* c0, const float* Wp, const float* bp, int T, int B, int H, int decoder, float* h_all,
                 float* c_all, float* act_all, float* rel_out, hipStream_t st) {
  SGG_CHECK_ARG(((uintptr_t)c_all & 15) == 0 && ((uintptr_t)act_all & 15) == 0,
                "sgg_lstm_fwd: c_all and act_all must be 16-byte aligned (H=%d)", H);
  const GenFwd a{rel, A, Whh, bias, h0, c0, Wp, bp, T, B, H, h_all, c_all, act_all, rel_out};
  const bool dec = decoder != 0, save = act_all != nullptr;
  switch (lstm_gen_tiles(H)) {
    case 1: return gen_launch_fwd<1>(a, dec, save, st);
    case 2: return gen_launch_fwd<2>(a, dec, save, st);
    case 3: return gen_launch_fwd<3>(a, dec, save, st);
    case 4: return gen_launch_fwd<4>(a, dec, save, st);
    case 5: return gen_launch_fwd<5>(a, dec, save, st);
    case 6: return gen_launch_fwd<6>(a, dec, save, st);
    case 7: return gen_launch_fwd<7>(a, dec, save, st);
    default: return gen_launch_fwd<8>(a, dec, save, st);
  }
}

int lstm_gen_bwd(const float* A, const float* Whh, const float* Wp, const float* c_all, const float* act_all,
                 const float* dh_last, const float* dout, int T, int B, int H, int decoder, float* dG, float* dh0,
                 float* drel_in, float* drel_tot, hipStream_t st) {
  SGG_CHECK_ARG(((uintptr_t)c_all & 15) == 0 && ((uintptr_t)act_all & 15) == 0,
                "sgg_lstm_bwd: c_all and act_all must be 16-byte aligned (H=%d)", H);
  const GenBwd a{A, Whh, Wp, c_all, act_all, dh_last, dout, T, B, H, dG, dh0, drel_in, drel_tot};
  const bool dec = decoder != 0;
  switch (lstm_gen_tiles(H)) {
    case 1: return gen_launch_bwd<1>(a, dec, st);
    case 2: return gen_launch_bwd<2>(a, dec, st);
    case 3: return gen_launch_bwd<3>(a, dec, st);
    case 4: return gen_launch_bwd<4>(a, dec, st);
    case 5: return gen_launch_bwd<5>(a, dec, st);
    case 6: return gen_launch_bwd<6>(a, dec, st);
    case 7: return gen_launch_bwd<7>(a, dec, st);
    default: return gen_launch_bwd<8>(a, dec, st);
  }
}

}  // namespace sgg
