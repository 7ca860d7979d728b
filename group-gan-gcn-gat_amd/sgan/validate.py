"""Validation pass of the training loop (reference scripts/train.py:487-568
check_accuracy, with cal_l2_losses / cal_ade / cal_fde :571-601), on the device.

Per batch the reference runs the generator, the discriminator twice, about
forty small torch ops (relative_to_abs, four torch.cat, the L2 sums, the
displacement and final displacement errors three ways, the BCE pair) and
reads nine values back with .item().  Here a batch is one generator forward,
ONE discriminator forward over [fake | real] (as GanTrainer's D-step forms
it) and ONE metrics launch (sgg_val_metrics, csrc/metrics.hip) that adds the
batch's sums into a device accumulator; the host reads that accumulator once,
after the last batch.  Nothing inside the loop waits for the device.

The host RNG streams are the reference's: the loader's shuffle and the
per-batch noise from the torch host generator, and per batch the two
random.uniform draws of gan_d_loss (losses.py:36-49).
"""
import random

import numpy as np
import torch

from . import _native as N
from . import kernels as K
from .evaluate import draw_sample_noise
from .losses import gan_d_loss
from .scene import SceneIndex

SLOTS = ("l2_abs", "l2_rel", "ade", "ade_l", "ade_nl", "fde", "fde_l", "fde_nl", "d_loss", "n_l", "n_nl")
assert len(SLOTS) == N.VAL_SLOTS


class ValSums:
    """The sums of a validation pass: a device accumulator of N.VAL_SLOTS
    doubles (include/sgg.h: sgg_val_metrics) and the counts the host knows
    from the batch shapes."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.acc = torch.zeros(N.VAL_SLOTS, dtype=torch.float64, device=self.device)
        self.work = None
        self.total_traj = 0
        self.loss_mask_sum = 0
        self.n_batches = 0

    def _work(self, lib, B):
        need = int(lib.sgg_val_metrics_work_floats(B))
        if self.work is None or self.work.numel() < need:
            # (zeroed: the ticket word; calls are stream-ordered, so the old buffer is done with)
            self.work = torch.zeros(need, dtype=torch.float32, device=self.device)
        return self.work

    def add(self, pred_rel, batch, obs_len, scores=None, y_real=0.0):
        """One sgg_val_metrics launch: the sums of a batch (the reference's
        11-tuple, on the device) for the generator output pred_rel
        (pred_len, B, 2); scores (2B, [fake | real]) adds the discriminator
        loss with the real label y_real.  No host synchronisation."""
        lib = N.load()
        pred_gt, pred_gt_rel, non_linear, loss_mask = batch[1], batch[3], batch[8], batch[9]
        T, B = int(pred_rel.shape[0]), int(pred_rel.shape[1])
        f32 = lambda t: t.to(self.device, torch.float32)
        pred_rel, gt, gt_rel = f32(pred_rel).contiguous(), f32(pred_gt).contiguous(), f32(pred_gt_rel).contiguous()
        start = f32(batch[0][-1]).contiguous()
        nl = f32(non_linear).contiguous().view(-1)
        mask = f32(loss_mask)[:, obs_len:]
        if mask.stride(1) != 1 or (B > 1 and mask.stride(0) < T):
            mask = mask.contiguous()
        ld = int(mask.stride(0)) if B > 1 else max(int(mask.stride(0)), T)   # (one row: its stride is never used)
        # the kernel indexes without bounds beyond (T, B, ld): shapes checked here
        if not (tuple(pred_rel.shape) == tuple(gt.shape) == tuple(gt_rel.shape) == (T, B, 2)
                and tuple(start.shape) == (B, 2) and nl.numel() == B and tuple(mask.shape) == (B, T)):
            raise ValueError("ValSums.add: pred_rel %s, gt %s, gt_rel %s, start %s, non_linear %s, mask %s"
                             % (tuple(pred_rel.shape), tuple(gt.shape), tuple(gt_rel.shape), tuple(start.shape),
                                tuple(nl.shape), tuple(mask.shape)))
        if scores is not None:
            scores = f32(scores).contiguous().view(-1)
            if scores.numel() != 2 * B:
                raise ValueError("ValSums.add: %d scores for %d peds ([fake | real])" % (scores.numel(), B))
        N.check(lib.sgg_val_metrics(N.ptr(pred_rel), N.ptr(gt), N.ptr(gt_rel), N.ptr(start), N.ptr(mask), ld,
                                    N.ptr(nl), N.ptr(scores), float(y_real), T, B, N.ptr(self.acc),
                                    N.ptr(self._work(lib, B)), N.stream_ptr()), "sgg_val_metrics")
        self.total_traj += B
        self.loss_mask_sum += B * T          # torch.numel of the sliced mask (train.py:540)
        self.n_batches += 1

    def add_d_loss(self, value):
        """A discriminator loss formed outside the kernel (a device scalar)."""
        self.acc[8] += value.detach().to(self.device, torch.float64).reshape(())

    def read(self):
        """The pass's one device-to-host copy: the eleven sums by name, and
        the host-known total_traj, loss_mask_sum, n_batches."""
        out = dict(zip(SLOTS, self.acc.cpu().tolist()))
        out.update(total_traj=self.total_traj, loss_mask_sum=self.loss_mask_sum, n_batches=self.n_batches)
        return out


def reference_metrics(s, pred_len):
    """The dict scripts/train.py:547-568 returns, from the separated sums
    s = ValSums.read().  The reference creates its lists as `([],) * 2` and
    `([],) * 3` (train.py:490-492), so the names of a group are ONE list:
    both L2 entries hold both sums, and every ade* (fde*) entry the sum of
    all three displacement (final displacement) errors."""
    l2 = s["l2_abs"] + s["l2_rel"]
    ade = s["ade"] + s["ade_l"] + s["ade_nl"]
    fde = s["fde"] + s["fde_l"] + s["fde_nl"]
    m = {"d_loss": s["d_loss"] / s["n_batches"],
         "g_l2_loss_abs": l2 / s["loss_mask_sum"], "g_l2_loss_rel": l2 / s["loss_mask_sum"],
         "ade": ade / (s["total_traj"] * pred_len), "fde": fde / s["total_traj"]}
    for tag, n in (("l", s["n_l"]), ("nl", s["n_nl"])):
        m["ade_" + tag] = ade / (n * pred_len) if n != 0 else 0
        m["fde_" + tag] = fde / n if n != 0 else 0
    return m


def check_accuracy(args, loader, generator, discriminator, d_loss_fn=None, limit=False, device="cuda", raw=False):
    """Drop-in for scripts/train.py:487-568.

    loader yields the reference's 11-tuples or (11-tuple, SceneIndex) pairs
    (sgan.data.device.DeviceLoader).  d_loss_fn None or sgan.losses.gan_d_loss
    takes the fused path (the loss is formed in the metrics launch, with
    gan_d_loss's two random.uniform draws made here); any other callable is
    applied to (scores_real, scores_fake) and its value accumulated on the
    device.  limit stops after the batch that brings the ped count to
    args.num_samples_check.  The generator runs in eval mode and is put back
    in train mode, as in the reference.

    Returns the reference's dict -- the values of every checkpoint's
    metrics_val / metrics_train history, which min_ade / min_ade_nl select
    on.  As the reference runs, these are NOT the separated metrics:
    train.py:490-492 binds the names of each group to one list, so
      g_l2_loss_abs == g_l2_loss_rel == (sum abs + sum rel) / loss_mask_sum,
      ade, ade_l, ade_nl share the numerator sum ade + sum ade_l + sum ade_nl
      (divided by total_traj, linear and non-linear peds times pred_len),
      fde, fde_l, fde_nl likewise,
    and ade_l / fde_l (ade_nl / fde_nl) are the integer 0 when the pass saw no
    linear (non-linear) ped.  raw=True returns ValSums.read() instead: the
    separated sums and counts, from which the true ADE is sums["ade"] /
    (total_traj * pred_len)."""
    sums = ValSums(device)
    fused = d_loss_fn is None or d_loss_fn is gan_d_loss
    generator.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                if len(batch) == 2:      # DeviceLoader: (11-tuple on the device, SceneIndex)
                    batch, sc = batch
                else:
                    sc = SceneIndex.from_seq_start_end(batch[-1], device)   # host seq_start_end: no sync
                batch = [t.to(device, non_blocking=True) for t in batch]
                obs, obs_rel, pred_gt_rel, obs_g, sse = batch[0], batch[2], batch[3], batch[6], batch[10]
                B = obs.size(1)
                z = draw_sample_noise(generator, sc, B, 1)   # the forward's own host draw (models.py:827-835)
                fake_rel = generator(obs, obs_rel, sse, obs_g, user_noise=z, scenes=sc)
                # D reads traj[0] and traj_rel only: [fake | real] side by side, one forward
                traj_rel, start = K.traj_cat(obs_rel, fake_rel, pred_gt_rel, obs[0])
                sc2 = sc.repeat(2)
                sse2 = torch.from_numpy(np.stack([sc2.host_off[:-1], sc2.host_off[1:]], 1))
                scores = discriminator(start, traj_rel, sse2, scenes=sc2)
                if fused:
                    y_real = random.uniform(0.7, 1.2)
                    random.uniform(0, 0.3)   # the fake-label draw (losses.py:47): zeros_like * y == 0
                    sums.add(fake_rel, batch, args.obs_len, scores, y_real)
                else:
                    sums.add(fake_rel, batch, args.obs_len)
                    sums.add_d_loss(d_loss_fn(scores[B:], scores[:B]))
                if limit and sums.total_traj >= args.num_samples_check:
                    break
    finally:
        generator.train()
    s = sums.read()
    return s if raw else reference_metrics(s, args.pred_len)
