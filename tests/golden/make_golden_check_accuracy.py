"""Golden fixture of the validation pass, from the reference code.

    python tests/golden/make_golden_check_accuracy.py

check_accuracy.json  the reference's own check_accuracy (scripts/train.py
                     :487-568) with its own gan_d_loss and its own
                     data_loader, on the models make_golden.py builds (the
                     committed weights.npz), over the shipped
                     tests/golden/datasets_group splits.  Per case: the
                     arguments, the returned dict, the number of batches the
                     loop consumed, and the host stream positions right after
                     the call -- random.random() and torch.rand(1).

Cases (SEED seeds torch and random right before each call):
    gat/eth          one whole split, unlimited: eth/test is the smallest
                     (70 sequences: one full batch of 64 and a ragged one of 6)
    gat/zara1_train  limit=True on zara1/train, num_samples_check one above
                     the ped count of the first two batches, so the loop stops
                     after its third batch
    gat/zara1_b100   zara1/test at batch 100: 602 sequences leave a last batch of 2
    gcn/hotel        the gcn family (models.py:902's commented call, as
                     make_golden.py evaluates it), hotel/test: 301 sequences,
                     a last batch of 45

The reference's dataset lists a split's files in the file system's order;
here it is handed the sorted listing (sorted_listing below), the order in
which sgan.data reads them.  Nothing of the reference is copied: it is
called.  About half a minute on a CPU.
"""
import json
import os
import random
import types

import torch

from make_golden import ARGS, DL, EV, HERE, TR, _gen_forward, build_models

SEED = 2024
CASES = [   # name, family, split, dset_type, batch_size, limit
    ("gat/eth", "gat", "eth", "test", 64, False),
    ("gat/zara1_train", "gat", "zara1", "train", 64, True),
    ("gat/zara1_b100", "gat", "zara1", "test", 100, False),
    ("gcn/hotel", "gcn", "hotel", "test", 64, False),
]


class Counting:
    """A loader that counts the batches drawn from it."""

    def __init__(self, loader):
        self.loader, self.n = loader, 0

    def __iter__(self):
        for b in self.loader:
            self.n += 1
            yield b


def sorted_listing(fn, *args):
    """fn(*args) with os.listdir returning sorted names: the reference's
    dataset reads a split's files in os.listdir order, which is the file
    system's; a split of several files (zara1/train has seven) then numbers
    its sequences differently from one machine to the next.  The package's
    dataset reads them sorted, so the fixture does too."""
    listdir = os.listdir
    os.listdir = lambda *a, **k: sorted(listdir(*a, **k))
    try:
        return fn(*args)
    finally:
        os.listdir = listdir


def seed_all():
    torch.manual_seed(SEED)
    random.seed(SEED)


def main():
    res = {}
    for name, family, split, dset_type, bs, limit in CASES:
        g, d = build_models(0)
        if family == "gcn":
            g.forward = types.MethodType(
                lambda self, ot, orl, sse, og, user_noise=None: _gen_forward(
                    self, dict(obs_traj=ot, obs_traj_rel=orl, seq_start_end=sse, obs_traj_g=og), user_noise, "gcn"), g)
        a = EV.AttrDict(dict(vars(ARGS)))
        a["batch_size"] = bs
        _, loader = sorted_listing(DL.data_loader, a, os.path.join(HERE, "datasets_group", split, dset_type))
        if limit:   # the batches' ped counts under this seed (the order is drawn when the iterator is made)
            seed_all()
            peds = [b[0].size(1) for b in loader]
            a["num_samples_check"] = peds[0] + peds[1] + 1
        seed_all()
        counted = Counting(loader)
        m = TR.check_accuracy(a, counted, g, d, TR.gan_d_loss, limit=limit)
        after = dict(random=random.random(), torch=float(torch.rand(1)))
        assert g.training
        if limit:
            assert counted.n == 3, counted.n
        res[name] = dict(family=family, split=split, dset_type=dset_type, batch_size=bs, limit=limit,
                         num_samples_check=int(a["num_samples_check"]), seed=SEED, n_batches=counted.n,
                         metrics={k: (v if isinstance(v, int) else float(v)) for k, v in m.items()}, after=after)
        print(name, res[name], flush=True)
    path = os.path.join(HERE, "check_accuracy.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
