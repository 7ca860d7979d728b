// Fused LSTM sequences: the Encoder (reference sgan/models.py:32-92) and the
// autoregressive Decoder rollout (models.py:142-178), forward and backward,
// one launch each instead of one MIOpen RNN call (plus Linear/cat kernels)
// per time step.  This file holds the C entry points (include/sgg.h): their
// argument checks and the choice between the two kernel families.
//
// Folding (exact up to fp32 reassociation): the input of every step is a
// 2-d relative displacement r embedded by Linear(2, E), so
//   W_ih (We r + be) + b_ih + b_hh = A r + b'    with A = W_ih We (4H x 2),
//                                                b' = W_ih be + b_ih + b_hh
// (A and b' are formed by the caller, sgg_fold_fwd, and sgg_fold_bwd carries
// their gradients back to W_ih, We, be, b_ih, b_hh).  Decoder: r_0 is the
// last observed displacement, r_t = Wp h_t + bp (hidden2pos) feeds step t+1.
//
// Families:
//  - four-wave MFMA kernels (lstm_mw.hip), every built H (16 / 32 / 48 / 64):
//    every forward that saves states, every backward (it reads the tile-native
//    states its forward wrote), and every forward the rollout does not claim;
//  - batch-MFMA rollout (lstm_mfma.hip): forwards without saved states where
//    lstm_fwd_mfma_ok (H = 32, B >= kLstmMfmaMinPeds), unless SGG_LSTM_NO_MFMA.
//  - generic kernels (lstm_gen.hip): every other 1 <= H <= 128, plain forms only
//    (sgg_lstm_fwd / sgg_lstm_bwd); the fused forms below stay four-wave only.
// H <= 0 and H > 128 are refused here, before any launch: the H switches of
// lstm_mw.hip have no error arm.
#include <stdlib.h>
#include <string.h>

#include "sgg_common.h"

using namespace sgg;

extern "C" long long sgg_lstm_state_floats(int T, int B, int H, int which) {
  if (T < 1 || B < 0 || (which != 0 && which != 1)) return -1;
  if (lstm_gen_ok(H)) return lstm_gen_state_floats(T, B, H, which);
  if (!lstm_mw_ok(H)) return -1;
  return lstm_mw_state_floats(T, B, H, which);
}

extern "C" long long sgg_lstm_dg_floats(int T, int B, int H) {
  if (T < 1 || B < 0 || !(lstm_gen_ok(H) || lstm_mw_ok(H))) return -1;
  return lstm_gen_ok(H) ? (long long)T * B * 4 * H : 0;
}

extern "C" const char* sgg_lstm_kernel_name(int H, int B, int decoder, int save, int bwd) {
  // mirrors the dispatch of sgg_lstm_fwd / sgg_lstm_bwd below (save = act_all
  // != NULL for the forward, = weight gradients in the kernel for the backward)
  static char buf[96];
  const char* tf[2] = {"false", "true"};
  if (lstm_gen_ok(H) && B > 0) {   // the generic family: the plain forward and backward only
    if (bwd > 1) return "";
    if (bwd) snprintf(buf, sizeof buf, "sgg::lstm_gen_bwd_kernel<%d, %s>", lstm_gen_tiles(H), tf[decoder != 0]);
    else snprintf(buf, sizeof buf, "sgg::lstm_gen_fwd_kernel<%d, %s, %s>", lstm_gen_tiles(H), tf[decoder != 0], tf[save != 0]);
    return buf;
  }
  if (!lstm_mw_ok(H) || B <= 0) return "";
  if (bwd == 3 || bwd == 4) {   // given a pooled-gradient source (sgg_lstm_bwd_pooldh)
    if (decoder || !lstm_mw_bwd_pdh_ok(H) || (bwd == 4 && (!save || !lstm_mw_bwd_nodx_ok(H)))) return "";
    if (bwd == 4) snprintf(buf, sizeof buf, "sgg::lstm_mw_bwd_nodx_pdh_kernel<%d>", H);
    else snprintf(buf, sizeof buf, "sgg::lstm_mw_bwd_pdh_kernel<%d, %s>", H, tf[save != 0]);
  } else if (bwd == 2) {   // the encoder's weight-gradient backward given no drel_in ("" where it is not built)
    if (decoder || !save || !lstm_mw_bwd_nodx_ok(H)) return "";
    snprintf(buf, sizeof buf, "sgg::lstm_mw_bwd_nodx_kernel<%d>", H);
  } else if (bwd) {
    snprintf(buf, sizeof buf, "sgg::lstm_mw_bwd_kernel<%d, %s, %s>", H, tf[decoder != 0], tf[save != 0]);
  } else if (!save && lstm_fwd_mfma_ok(H, B) && !getenv("SGG_LSTM_NO_MFMA")) {
    // (lstm_mfma.hip: the split-bf16 gate GEMM for H = 32 unless SGG_LSTM_X3=0)
    const char* x3e = getenv("SGG_LSTM_X3");
    const bool x3 = H == 32 && !(x3e && strcmp(x3e, "0") == 0);
    snprintf(buf, sizeof buf, "sgg::lstm_fwd_mfma_kernel<%d, %s, %s>", H, tf[x3], tf[decoder != 0]);
  } else {
    snprintf(buf, sizeof buf, "sgg::lstm_mw_fwd_kernel<%d, %s, %s>", H, tf[decoder != 0], tf[save != 0]);
  }
  return buf;
}

// the family sgg_lstm_fwd picks for these sizes is the four-wave one
static bool fwd_picks_mw(int H, int B, bool save) {
  return lstm_mw_ok(H) && (save || !lstm_fwd_mfma_ok(H, B) || getenv("SGG_LSTM_NO_MFMA"));
}

extern "C" int sgg_lstm_u_ok(int T, int B, int H, int decoder, int save, int NU) {
  return !decoder && B > 0 && T >= 1 && NU >= 16 && NU % 16 == 0 && fwd_picks_mw(H, B, save != 0);
}

extern "C" int sgg_lstm_fwd_u(const float* rel, const float* A, const float* Whh, const float* bias, const float* h0,
                              const float* c0, int T, int B, int H, float* h_all, float* c_all, float* act_all,
                              const float* Wu, int ldwu, const float* cu, int NU, float* U, void* stream) {
  SGG_CHECK_ARG(rel && A && Whh && bias && h_all && c_all && Wu && cu && U, "sgg_lstm_fwd_u: null pointer");
  SGG_CHECK_ARG(sgg_lstm_u_ok(T, B, H, 0, act_all != nullptr, NU) && ldwu >= H,
                "sgg_lstm_fwd_u: no projection epilogue for T=%d B=%d H=%d NU=%d ldwu=%d (sgg_lstm_u_ok)", T, B, H, NU,
                ldwu);
  return lstm_mw_fwd(rel, A, Whh, bias, h0, c0, nullptr, nullptr, T, B, H, 0, h_all, c_all, act_all, nullptr,
                     (hipStream_t)stream, Wu, ldwu, cu, NU, U);
}

extern "C" int sgg_lstm_bwd_split(const float* A, const float* Whh, const float* Wp, const float* h_all,
                                  const float* c_all, const float* act_all, const float* rel, const float* rel_out,
                                  const float* dout, const float* dout2, int bsplit, int T, int B, int H, float* dh0,
                                  float* drel_in, float* drel_tot, float* wpart, void* stream) {
  SGG_CHECK_ARG(A && Whh && Wp && h_all && c_all && act_all && rel && rel_out && dout && dout2 && drel_in && drel_tot,
                "sgg_lstm_bwd_split: null pointer");
  SGG_CHECK_ARG(T >= 1 && B >= 1 && bsplit >= 0 && bsplit <= B && lstm_mw_ok(H),
                "sgg_lstm_bwd_split: bad sizes or no four-wave kernel (T=%d B=%d H=%d bsplit=%d)", T, B, H, bsplit);
  return lstm_mw_bwd(A, Whh, Wp, h_all, c_all, act_all, rel, rel_out, nullptr, dout, T, B, H, 1, dh0, drel_in,
                     drel_tot, wpart, (hipStream_t)stream, dout2, bsplit);
}

extern "C" int sgg_lstm_bwd_tail(const float* A, const float* Whh, const float* h_all, const float* c_all,
                                 const float* act_all, const float* rel, const float* dh_last, int T, int B, int H,
                                 int t_stop, float* drel_in, void* stream) {
  SGG_CHECK_ARG(A && Whh && h_all && c_all && act_all && rel && drel_in, "sgg_lstm_bwd_tail: null pointer");
  SGG_CHECK_ARG(T >= 1 && B >= 1 && t_stop >= 0 && t_stop < T && lstm_mw_ok(H),
                "sgg_lstm_bwd_tail: bad sizes or no four-wave kernel (T=%d B=%d H=%d t_stop=%d)", T, B, H, t_stop);
  return lstm_mw_bwd(A, Whh, nullptr, h_all, c_all, act_all, rel, nullptr, dh_last, nullptr, T, B, H, 0, nullptr,
                     drel_in, nullptr, nullptr, (hipStream_t)stream, nullptr, 0, t_stop);
}

static MwSeg to_mw(const SggLstmSeg& s) {
  return MwSeg{s.rel, s.A, s.Whh, s.bias, s.h0, s.c0, nullptr, nullptr, s.T, s.B, s.Bl, s.t0, s.Tl, s.Bsrc,
               s.h_all, s.c_all, s.act_all, nullptr, s.Wu, s.ldwu, s.cu, s.NU, s.U};
}

extern "C" int sgg_lstm_fwd_seg(const SggLstmSeg* seg, int H, void* stream) {
  SGG_CHECK_ARG(seg, "sgg_lstm_fwd_seg: null segment");
  SGG_CHECK_ARG(lstm_mw_ok(H), "sgg_lstm_fwd_seg: no four-wave kernel for H=%d", H);
  return lstm_mw_fwd_seg(to_mw(*seg), H, (hipStream_t)stream);
}

static int device_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int d = 0, v = 0;
    const bool ok = hipGetDevice(&d) == hipSuccess &&
                    hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess;
    ncu = ok && v > 0 ? v : 256;
  }
  return ncu;
}

extern "C" int sgg_lstm_fwd_seg_glue(const SggLstmSeg* seg, int H, const SggGlueSeg* glue, void* stream) {
  SGG_CHECK_ARG(seg && glue, "sgg_lstm_fwd_seg_glue: null segment");
  SGG_CHECK_ARG(lstm_mw_ok(H), "sgg_lstm_fwd_seg_glue: no four-wave kernel for H=%d", H);
  const SggGlueSeg& g = *glue;
  SGG_CHECK_ARG(g.kind == SGG_GLUE_NONE || g.kind == SGG_GLUE_SELECT || g.kind == SGG_GLUE_L2BWD,
                "sgg_lstm_fwd_seg_glue: glue kind %d", g.kind);
  if (g.kind == SGG_GLUE_SELECT) {   // sgg_l2_select's rules
    SGG_CHECK_ARG(g.pred && g.gt && g.mask && g.scene_off && g.best, "sgg_lstm_fwd_seg_glue (select): null pointer");
    SGG_CHECK_ARG(g.S >= 0 && g.T >= 1 && g.B >= 0 && g.k >= 1 && g.k <= 256 && g.ldm >= g.T,
                  "sgg_lstm_fwd_seg_glue (select): bad sizes");
  } else if (g.kind == SGG_GLUE_L2BWD) {   // sgg_l2_loss_bwd_scenes' rules
    SGG_CHECK_ARG(g.pred && g.gt && g.mask && g.scene_off && g.gout && g.dpred,
                  "sgg_lstm_fwd_seg_glue (l2 backward): null pointer");
    SGG_CHECK_ARG(g.S >= 0 && g.T >= 1 && g.B >= 0 && g.ldm >= g.T && g.ldp >= 2 * g.B && g.ldd >= 2 * g.B,
                  "sgg_lstm_fwd_seg_glue (l2 backward): bad sizes");
  }
  // The glue workgroups ride where the segment's last round of workgroups leaves them CUs (the H = 48 kernels hold
  // one workgroup per CU).  Behind a grid that fills the device they would only lengthen its tail, two short
  // workgroups per CU one after the other, slower than their own launch (512 scenes, [12, 20480]: +8 us per
  // iteration): the glue body then goes first, in its stand-alone launch -- the same results either way.
  if (g.kind != SGG_GLUE_NONE && g.S > 0) {
    const int cus = device_cus(), nblk = (seg->B + 15) / 16, last = nblk % cus;
    if ((nblk >= cus && last == 0) || last + g.S > cus) {
      const int rc = g.kind == SGG_GLUE_SELECT
                         ? sgg_l2_select(g.pred, g.gt, g.mask, g.ldm, g.scene_off, g.S, g.T, g.B, g.k, g.best, stream)
                         : sgg_l2_loss_bwd_scenes(g.pred, g.ldp, g.gt, g.mask, g.ldm, g.scene_off, g.S, g.T, g.B, g.w,
                                                  g.gout, g.dpred, g.ldd, g.term, stream);
      if (rc) return rc;
      return lstm_mw_fwd_seg(to_mw(*seg), H, (hipStream_t)stream);
    }
  }
  return lstm_mw_fwd_seg(to_mw(*seg), H, (hipStream_t)stream, glue);
}

extern "C" int sgg_lstm_fwd_seg2(const SggLstmSeg* a, int Ha, const SggLstmSeg* b, int Hb, void* stream) {
  SGG_CHECK_ARG(a && b, "sgg_lstm_fwd_seg2: null segment");
  SGG_CHECK_ARG(lstm_mw_ok(Ha) && lstm_mw_ok(Hb), "sgg_lstm_fwd_seg2: no four-wave kernel (Ha=%d Hb=%d)",
                Ha, Hb);
  return lstm_mw_fwd_seg2(to_mw(*a), Ha, to_mw(*b), Hb, (hipStream_t)stream);
}

extern "C" int sgg_lstm_fwd_seg3(const SggLstmSeg* a, int Ha, const SggLstmSeg* b, int Hb, const SggLstmSeg* c, int Hc,
                                 void* stream) {
  SGG_CHECK_ARG(a && b && c, "sgg_lstm_fwd_seg3: null segment");
  SGG_CHECK_ARG(lstm_mw_ok(Ha) && lstm_mw_ok(Hb) && lstm_mw_ok(Hc),
                "sgg_lstm_fwd_seg3: no four-wave kernel (Ha=%d Hb=%d Hc=%d)", Ha, Hb, Hc);
  return lstm_mw_fwd_seg3(to_mw(*a), Ha, to_mw(*b), Hb, to_mw(*c), Hc, (hipStream_t)stream);
}

extern "C" int sgg_lstm_bwd_shared(const float* A, const float* Whh, const float* h_all, const float* c_all,
                                   const float* act_all, const float* rel, const float* dh_last, int T, int B, int H,
                                   int t_sh, int Bsrc, float* drel_in, float* wpart, void* stream) {
  SGG_CHECK_ARG(A && Whh && h_all && c_all && act_all && rel, "sgg_lstm_bwd_shared: null pointer");
  SGG_CHECK_ARG(T >= 1 && B >= 1 && t_sh >= 1 && lstm_mw_ok(H),
                "sgg_lstm_bwd_shared: bad sizes or no four-wave kernel (T=%d B=%d H=%d t_sh=%d)", T, B, H, t_sh);
  SGG_CHECK_ARG(drel_in || (wpart && lstm_mw_bwd_nodx_ok(H)),
                "sgg_lstm_bwd_shared: drel_in may be NULL only with weight gradients (wpart) and H = 16 / 32 / 48 "
                "(wpart=%d H=%d)", wpart != nullptr, H);
  return lstm_mw_bwd(A, Whh, nullptr, h_all, c_all, act_all, rel, nullptr, dh_last, nullptr, T, B, H, 0, nullptr,
                     drel_in, nullptr, wpart, (hipStream_t)stream, nullptr, 0, 0, t_sh, Bsrc);
}

extern "C" int sgg_lstm_bwd_pooldh_ok(int H) { return lstm_mw_bwd_pdh_ok(H); }

// Where the prologue pays: the backward's workgroups come in ONE round (16 peds each, <= one per CU).  The launch is
// then a dependency chain beside idle CUs, and the product's 4 - 5 us in one chain cost less than the 7 - 10 us
// launch they replace.  A grid of several rounds pays the prologue once per round, while the launch it replaces
// filled the device: 512 scenes of 20 peds (1,280 and 640 workgroups), +19 us per iteration.
extern "C" int sgg_lstm_bwd_pooldh_pays(int B, int H) {
  return B >= 1 && lstm_mw_bwd_pdh_ok(H) && (B + 15) / 16 <= device_cus();
}

// The h^T dU workgroups ride where the recurrence's workgroups come in ONE round that leaves CUs free, and the
// riders pass over those free CUs in at most four rounds: a recurrence workgroup is then the launch's long pole
// (10 - 40 us against a rider's 2 - 3), and the riders are done long before it (the H = 48 forms hold one
// workgroup per CU, so a rider finds no place beside a recurrence workgroup).  Behind a carrier that fills the
// device they would be dispatched last and only lengthen its tail (the glue riders' finding,
// sgg_lstm_fwd_seg_glue): there the partials keep their own launch.
extern "C" int sgg_lstm_bwd_pooldh_rides(int B, int H, int NU) {
  if (B < 1 || !lstm_mw_bwd_pdh_ok(H) || NU < 1) return 0;
  const char* e = getenv("SGG_POOL_DH_RIDE");   // "0": the partials always take their own launch (A/B runs)
  if (e && e[0] == '0') return 0;
  const int cus = device_cus(), nblk = (B + 15) / 16;
  const int riders = ((H + 63) / 64) * ((NU + 63) / 64) * sgg_xtw_splits(B, H, NU);
  return nblk < cus && riders <= 4 * (cus - nblk);
}

extern "C" int sgg_lstm_bwd_pooldh(const float* A, const float* Whh, const float* h_all, const float* c_all,
                                   const float* act_all, const float* rel, const SggPoolDh* src, int T, int B, int H,
                                   int t_stop, int t_sh, int Bsrc, float* dh0, float* drel_in, float* wpart,
                                   void* stream) {
  SGG_CHECK_ARG(A && Whh && h_all && c_all && act_all && rel && src && src->dU && src->W1h,
                "sgg_lstm_bwd_pooldh: null pointer");
  SGG_CHECK_ARG(lstm_mw_bwd_pdh_ok(H), "sgg_lstm_bwd_pooldh: no pooled-gradient prologue for H=%d (32 / 48)", H);
  SGG_CHECK_ARG(T >= 1 && B >= 1 && t_stop >= 0 && t_stop < T && t_sh >= 0, "sgg_lstm_bwd_pooldh: bad sizes T=%d B=%d "
                "t_stop=%d t_sh=%d", T, B, t_stop, t_sh);
  SGG_CHECK_ARG(src->NU >= 256 && src->ldu >= src->NU && src->ldw >= H,
                "sgg_lstm_bwd_pooldh: bad source sizes NU=%d ldu=%d ldw=%d (NU >= 256: sgg_xw's split-K form)", src->NU,
                src->ldu, src->ldw);
  SGG_CHECK_ARG(t_stop == 0 || (!wpart && !dh0 && t_sh == 0),
                "sgg_lstm_bwd_pooldh: t_stop > 0 is the input-gradient form (no wpart, dh0 or shared prefix)");
  SGG_CHECK_ARG(drel_in || (wpart && lstm_mw_bwd_nodx_ok(H)),
                "sgg_lstm_bwd_pooldh: drel_in may be NULL only with weight gradients (wpart)");
  int ride = 0;
  if (src->ws) {
    SGG_CHECK_ARG(wpart && src->h && src->ldh >= H, "sgg_lstm_bwd_pooldh: the h^T dU partials need wpart and h");
    const int splits = sgg_xtw_splits(B, H, src->NU);
    const size_t need = sizeof(float) * (size_t)splits * ((size_t)H * src->NU + src->NU);
    SGG_CHECK_ARG(src->splits == splits && src->ws_bytes >= need,
                  "sgg_lstm_bwd_pooldh: splits %d (sgg_xtw_splits: %d), workspace %zu < %zu bytes", src->splits, splits,
                  src->ws_bytes, need);
    ride = sgg_lstm_bwd_pooldh_rides(B, H, src->NU);
    if (!ride)
      if (int rc = sgg_xtw_partial(src->h, src->ldh, src->dU, src->ldu, nullptr, 0, B, H, src->NU, 1, src->ws,
                                   src->ws_bytes, stream))
        return rc;
  }
  return lstm_mw_bwd(A, Whh, nullptr, h_all, c_all, act_all, rel, nullptr, nullptr, nullptr, T, B, H, 0, dh0, drel_in,
                     nullptr, wpart, (hipStream_t)stream, nullptr, 0, t_stop, t_sh, Bsrc, src, ride);
}

extern "C" int sgg_lstm_wpart_rows(int H, int B) {
  if (B < 0 || !(lstm_gen_ok(H) || lstm_mw_ok(H))) return -1;
  return lstm_mw_wpart_rows(H, B);   // (one row per 16 peds in either family; the generic one writes dG, no slab)
}

extern "C" int sgg_lstm_fwd(const float* rel, const float* A, const float* Whh, const float* bias, const float* h0,
                            const float* c0, const float* Wp, const float* bp, int T, int B, int H, int decoder, float* h_all,
                            float* c_all, float* act_all, float* rel_out, void* stream) {
  SGG_CHECK_ARG(rel && A && Whh && bias && h_all && c_all, "sgg_lstm_fwd: null pointer");
  SGG_CHECK_ARG(!decoder || (Wp && bp && rel_out), "sgg_lstm_fwd: decoder needs Wp, bp, rel_out");
  SGG_CHECK_ARG(T >= 1 && B >= 0, "sgg_lstm_fwd: bad sizes T=%d B=%d", T, B);
  if (B == 0) return 0;
  SGG_CHECK_ARG(lstm_mw_ok(H) || lstm_gen_ok(H), "sgg_lstm_fwd: hidden size %d (1 .. 128)", H);
  hipStream_t st = (hipStream_t)stream;
  if (lstm_gen_ok(H))
    return lstm_gen_fwd(rel, A, Whh, bias, h0, c0, Wp, bp, T, B, H, decoder, h_all, c_all, act_all, rel_out, st);
  // the MFMA rollout only without saved states (inference / no-grad samples):
  // saved states are the four-wave family's, read back by its backward
  if (!act_all && lstm_fwd_mfma_ok(H, B) && !getenv("SGG_LSTM_NO_MFMA"))
    return lstm_fwd_mfma(rel, A, Whh, bias, h0, c0, Wp, bp, T, B, H, decoder, h_all, c_all, nullptr, rel_out, st);
  return lstm_mw_fwd(rel, A, Whh, bias, h0, c0, Wp, bp, T, B, H, decoder, h_all, c_all, act_all, rel_out, st);
}

static int dec_check(const SggDecInit* di, const float* A, const float* Whh, const float* bias, const float* Wp,
                     const float* bp, int T, int B, int H, float* h_all, float* c_all, float* act_all, float* rel_out,
                     const SggTrajOut* to) {
  SGG_CHECK_ARG(di && di->ctx && di->ped_scene && di->last_rel && (di->nz == 0 || di->z) && A && Whh && bias &&
                    ((h_all && c_all) || (!h_all && !c_all && !act_all)) && Wp && bp && rel_out,
                "sgg_lstm_fwd_dec: null pointer");
  SGG_CHECK_ARG(T >= 1 && B >= 0 && di->Bper >= 1 && B % di->Bper == 0 && di->Dc >= 1 && di->nz >= 0 &&
                    di->Dc + di->nz == H && di->ldc >= di->Dc && di->S >= 1,
                "sgg_lstm_fwd_dec: bad sizes (T=%d B=%d Bper=%d Dc=%d nz=%d H=%d)", T, B, di->Bper, di->Dc, di->nz, H);
  if (to) {
    SGG_CHECK_ARG(to->out && to->head && (!to->start || to->pos0), "sgg_lstm_fwd_dec: null pointer in SggTrajOut");
    SGG_CHECK_ARG(to->T0 >= 0 && to->ncol >= 1 && to->col0 >= 0 && to->col0 + to->ncol <= B &&
                      to->NB == (to->b ? 2 : 1) * to->ncol && to->ldh >= 2 * to->ncol &&
                      (!to->b || to->ldb >= 2 * to->ncol),
                  "sgg_lstm_fwd_dec: bad SggTrajOut sizes (NB=%d T0=%d col0=%d ncol=%d B=%d)", to->NB, to->T0,
                  to->col0, to->ncol, B);
  }
  return 0;
}

extern "C" int sgg_lstm_fwd_dec_seg(const SggDecInit* di, const float* A, const float* Whh, const float* bias,
                                    const float* Wp, const float* bp, int T, int B, int H, float* h_all, float* c_all,
                                    float* act_all, float* rel_out, float* rel0_out, const SggTrajOut* to,
                                    const SggLstmSeg* pre, int Hp, void* stream) {
  if (int rc = dec_check(di, A, Whh, bias, Wp, bp, T, B, H, h_all, c_all, act_all, rel_out, to)) return rc;
  SGG_CHECK_ARG(pre && B >= 1 && act_all && lstm_mw_ok(H) && lstm_mw_ok(Hp),
                "sgg_lstm_fwd_dec_seg: needs a saving four-wave decoder and a prefix segment (H=%d B=%d Hp=%d)", H, B,
                Hp);
  return lstm_mw_fwd_dec_seg(A, Whh, bias, Wp, bp, T, B, H, h_all, c_all, act_all, rel_out, di, rel0_out, to,
                             to_mw(*pre), Hp, (hipStream_t)stream);
}

extern "C" int sgg_lstm_fwd_dec2(const SggDecInit* di, const SggDecInit* di2, const float* A, const float* Whh,
                                 const float* bias, const float* Wp, const float* bp, int T, int B, int B2, int H,
                                 float* rel_out, float* rel_out2, const SggTrajOut* to2, void* stream) {
  if (int rc = dec_check(di, A, Whh, bias, Wp, bp, T, B, H, nullptr, nullptr, nullptr, rel_out, nullptr)) return rc;
  if (int rc = dec_check(di2, A, Whh, bias, Wp, bp, T, B2, H, nullptr, nullptr, nullptr, rel_out2, to2)) return rc;
  SGG_CHECK_ARG(B >= 1 && B2 >= 1 && lstm_fwd_mfma_ok(H, B) && !getenv("SGG_LSTM_NO_MFMA"),
                "sgg_lstm_fwd_dec2: the batch-MFMA rollout family only (H=%d B=%d)", H, B);
  return lstm_fwd_mfma_dec2(di, di2, A, Whh, bias, Wp, bp, T, B, B2, H, rel_out, rel_out2, to2, (hipStream_t)stream);
}

extern "C" int sgg_lstm_fwd_dec(const SggDecInit* di, const float* A, const float* Whh, const float* bias,
                                const float* Wp, const float* bp, int T, int B, int H, float* h_all, float* c_all,
                                float* act_all, float* rel_out, float* rel0_out, const SggTrajOut* to,
                                void* stream) {
  if (int rc = dec_check(di, A, Whh, bias, Wp, bp, T, B, H, h_all, c_all, act_all, rel_out, to)) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (!act_all && lstm_fwd_mfma_ok(H, B) && !getenv("SGG_LSTM_NO_MFMA")) {
    if (to) {   // the batch-MFMA family writes the discriminator input as a second segment (alone here)
      SGG_CHECK_ARG(!h_all, "sgg_lstm_fwd_dec: the batch-MFMA family writes the discriminator input without a "
                            "final state (h_all NULL)");
      return lstm_fwd_mfma_dec2(di, di, A, Whh, bias, Wp, bp, T, 0, B, H, nullptr, rel_out, to, st);
    }
    return lstm_fwd_mfma(nullptr, A, Whh, bias, nullptr, nullptr, Wp, bp, T, B, H, 1, h_all, c_all, nullptr, rel_out,
                         st, di);
  }
  // (a hidden size that is not built: the caller runs sgg_decoder_init + sgg_lstm_fwd, which names it)
  SGG_CHECK_ARG(!to || lstm_mw_ok(H), "sgg_lstm_fwd_dec: no family writes the discriminator input for H=%d B=%d", H,
                B);
  SGG_CHECK_ARG(lstm_mw_ok(H), "sgg_lstm_fwd_dec: no fused decoder start for H=%d B=%d (use sgg_decoder_init)", H, B);
  return lstm_mw_fwd(nullptr, A, Whh, bias, nullptr, nullptr, Wp, bp, T, B, H, 1, h_all, c_all, act_all, rel_out, st,
                     nullptr, 0, nullptr, 0, nullptr, di, act_all ? rel0_out : nullptr, to);
}

extern "C" int sgg_lstm_bwd(const float* A, const float* Whh, const float* Wp, const float* h_all, const float* c_all,
                            const float* act_all, const float* rel, const float* rel_out, const float* dh_last,
                            const float* dout, int T, int B, int H, int decoder, float* dG, float* dh0,
                            float* drel_in, float* drel_tot, float* wpart, void* stream) {
  SGG_CHECK_ARG(A && Whh && c_all && act_all, "sgg_lstm_bwd: null pointer");
  SGG_CHECK_ARG(drel_in || (!decoder && wpart && lstm_mw_bwd_nodx_ok(H)),
                "sgg_lstm_bwd: drel_in may be NULL only for an encoder of the four-wave family with weight gradients "
                "(wpart) and H = 16 / 32 / 48 (decoder=%d wpart=%d H=%d)", decoder, wpart != nullptr, H);
  SGG_CHECK_ARG(!decoder || (Wp && dout && drel_tot), "sgg_lstm_bwd: decoder needs Wp, dout, drel_tot");
  SGG_CHECK_ARG(T >= 1 && B >= 0, "sgg_lstm_bwd: bad sizes");
  if (B == 0) return 0;
  SGG_CHECK_ARG(lstm_mw_ok(H) || lstm_gen_ok(H), "sgg_lstm_bwd: hidden size %d (1 .. 128)", H);
  if (lstm_gen_ok(H))   // the recurrence only: the gate gradients go to dG, no slab is written (sgg.h)
    return lstm_gen_bwd(A, Whh, Wp, c_all, act_all, dh_last, dout, T, B, H, decoder, dG, dh0, drel_in, drel_tot,
                        (hipStream_t)stream);
  SGG_CHECK_ARG(!wpart || (h_all && rel && (!decoder || rel_out)),
                "sgg_lstm_bwd: weight gradients need h_all, rel (and rel_out for the decoder)");
  (void)dG;   // the four-wave family forms the weight gradients in the kernel: ignored
  return lstm_mw_bwd(A, Whh, Wp, h_all, c_all, act_all, rel, rel_out, dh_last, dout, T, B, H, decoder, dh0, drel_in,
                     drel_tot, wpart, (hipStream_t)stream);
}
