"""A plain restatement of the reference's validation loop (scripts/train.py
:487-568 check_accuracy with cal_l2_losses / cal_ade / cal_fde :571-601) in
torch ops: per batch one generator forward, two discriminator forwards,
relative_to_abs, four torch.cat, the losses of sgan.losses, and nine .item()
reads plus the two ped counts.  It runs on any modules with the reference's
call signatures (the CPU oracle's, the GPU package's) on whatever device they
live on, and is the CPU yardstick of tests/golden/check_accuracy.json and the
timing baseline of tools/bench_kernels.py validate.  Not a test module, not
product code.

The aliasing is the reference's: train.py:490-492 creates its lists as
`([],) * 2` and `([],) * 3`, so the two L2 names are ONE list, and so are the
three displacement and the three final displacement names.  Here that is
said outright: one list per group, every member's value appended to it."""
import torch

from sgan.losses import displacement_error, final_displacement_error, gan_d_loss, l2_loss
from sgan.utils import relative_to_abs


def check_accuracy_ref(args, loader, generator, discriminator, d_loss_fn=gan_d_loss, limit=False, device=None):
    d_vals, l2_vals, ade_vals, fde_vals = [], [], [], []   # (one list per aliased group)
    n_all, n_lin, n_nl, mask_numel = 0, 0, 0, 0
    generator.eval()
    with torch.no_grad():
        for batch in loader:
            if len(batch) == 2:   # a DeviceLoader's (11-tuple, SceneIndex): the tuple
                batch = batch[0]
            if device is not None:
                batch = [t.to(device) for t in batch]
            obs, gt, obs_rel, gt_rel, _ov, _pv, obs_g, _pg, nl, mask, sse = batch
            lin = 1 - nl
            mask = mask[:, args.obs_len:]
            fake_rel = generator(obs, obs_rel, sse, obs_g)
            fake = relative_to_abs(fake_rel, obs[-1])
            l2 = (l2_loss(fake, gt, mask, mode="sum"), l2_loss(fake_rel, gt_rel, mask, mode="sum"))
            ade = [displacement_error(fake, gt, w) for w in (None, lin, nl)]
            fde = [final_displacement_error(fake[-1], gt[-1], w) for w in (None, lin, nl)]
            s_fake = discriminator(torch.cat([obs, fake], 0), torch.cat([obs_rel, fake_rel], 0), sse)
            s_real = discriminator(torch.cat([obs, gt], 0), torch.cat([obs_rel, gt_rel], 0), sse)
            d_vals.append(d_loss_fn(s_real, s_fake).item())
            l2_vals += [v.item() for v in l2]
            ade_vals += [v.item() for v in ade]
            fde_vals += [v.item() for v in fde]
            mask_numel += torch.numel(mask)
            n_all += gt.size(1)
            n_lin += torch.sum(lin).item()
            n_nl += torch.sum(nl).item()
            if limit and n_all >= args.num_samples_check:
                break
    generator.train()
    T = args.pred_len
    m = {"d_loss": sum(d_vals) / len(d_vals),
         "g_l2_loss_abs": sum(l2_vals) / mask_numel, "g_l2_loss_rel": sum(l2_vals) / mask_numel,
         "ade": sum(ade_vals) / (n_all * T), "fde": sum(fde_vals) / n_all}
    for tag, n in (("l", n_lin), ("nl", n_nl)):   # an empty class reports the integer 0
        m["ade_" + tag] = sum(ade_vals) / (n * T) if n != 0 else 0
        m["fde_" + tag] = sum(fde_vals) / n if n != 0 else 0
    return m
