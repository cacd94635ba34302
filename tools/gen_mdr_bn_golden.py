"""Generate tests/golden/mdr_bn/*.npz by running the REFERENCE's MDR_BatchNorm inside the loop of its Star_Net (CPU; build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_mdr_bn_golden.py          # writes tests/golden/mdr_bn/*.npz

The reference (`/root/reference`, read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the
stand-in packages of oracle/shims/ on sys.path.  The class is the reference's own (models/submodules.py:107-175); the loop
around it restates models/star.py:147-154: select the rows of a scenario with a boolean mask, run that scenario's module,
write the rows back.  Recorded per case (arrays only; fp32 unless stated):

  x [3,B,C], ids [B] int64 (offset included), offset, w [B,C]    three batches, the scenario ids, the upstream weights
  weight, bias [S,C], shared_weight, shared_bias [C]           parameter values the modules are set to (random, so every gradient shows)
  init/bns.{i}.<key>, init1/<key>                              state_dict() of a fresh ModuleList / a fresh single module
  <tag>/y1                                                     training-mode output of the first step
  <tag>/buf{1,3}/running_mean, running_var [S,C], nbt [S]      buffers after 1 and 3 training steps
  <tag>/y_eval                                                 evaluation-mode output on x[0] after the three steps
  grad_train/<name>, grad_eval/<name>                          gradients of sum(y * w): first training step; evaluation after 3 steps (m01)
with <tag> = m01 (momentum 0.1) or cma (momentum None: cumulative average).
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402,F401  (puts the shims and the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from models.submodules import MDR_BatchNorm  # noqa: E402  (the reference)

# name -> C, offset, ids (before the offset).  S = 5 in `ragged`: scenario 4 empty, scenario 2 exactly two rows.
CASES = {
    "even": dict(C=5, S=3, offset=0, ids=[0, 1, 2, 2, 1, 0, 1, 2, 0, 0, 1, 2, 2, 2, 1, 0, 1, 1, 2, 0, 0, 2, 1]),
    "ragged": dict(C=33, S=5, offset=1, ids=([0, 1, 3, 3, 1, 0, 3] * 6)[:40]),
}
RAGGED_TWO = (5, 21)      # rows of `ragged` moved into scenario 2


def star_loop(bns, x, ids, offset, sw, sb):
    out = torch.zeros_like(x)
    for d, bn in enumerate(bns):
        rows = ids == d + offset
        out[rows] = bn(x[rows], sw, sb)
    return out


def run_case(name, outdir):
    cfg = CASES[name]
    C, S, offset = cfg["C"], cfg["S"], cfg["offset"]
    ids = torch.tensor(cfg["ids"])
    if name == "ragged":
        ids[list(RAGGED_TWO)] = 2
    ids = ids + offset
    B = ids.numel()
    rng = np.random.RandomState(sum(map(ord, name)))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))      # noqa: E731
    x = f32(rng.randn(3, B, C) * (0.5 + rng.rand(C)) + rng.randn(C) * 2)
    w = f32(rng.randn(B, C))
    weight, bias = f32(1 + 0.3 * rng.randn(S, C)), f32(0.3 * rng.randn(S, C))
    sw0, sb0 = f32(1 + 0.3 * rng.randn(C)), f32(0.3 * rng.randn(C))
    out = dict(x=x.numpy(), ids=ids.numpy(), offset=np.array(offset), w=w.numpy(), weight=weight.numpy(), bias=bias.numpy(),
               shared_weight=sw0.numpy(), shared_bias=sb0.numpy())
    holder = nn.Module()
    holder.bns = nn.ModuleList([MDR_BatchNorm(C) for _ in range(S)])
    for k, t in holder.state_dict().items():
        out[f"init/{k}"] = t.numpy().copy()
    for k, t in MDR_BatchNorm(C).state_dict().items():
        out[f"init1/{k}"] = t.numpy().copy()
    for tag, momentum in (("m01", 0.1), ("cma", None)):
        bns = nn.ModuleList([MDR_BatchNorm(C, momentum=momentum) for _ in range(S)])
        with torch.no_grad():
            for s, bn in enumerate(bns):
                bn.weight.copy_(weight[s])
                bn.bias.copy_(bias[s])
        sw, sb = sw0.clone().requires_grad_(True), sb0.clone().requires_grad_(True)

        def grads(y, xin, prefix):
            (y * w).sum().backward()
            out[f"{prefix}/x"] = xin.grad.numpy().copy()
            out[f"{prefix}/weight"] = np.stack([bn.weight.grad.numpy() for bn in bns])
            out[f"{prefix}/bias"] = np.stack([bn.bias.grad.numpy() for bn in bns])
            out[f"{prefix}/shared_weight"], out[f"{prefix}/shared_bias"] = sw.grad.numpy().copy(), sb.grad.numpy().copy()
            for p in [sw, sb] + list(bns.parameters()):
                p.grad = None

        bns.train()
        for step in (1, 2, 3):
            xin = x[step - 1].clone().requires_grad_(True)
            y = star_loop(bns, xin, ids, offset, sw, sb)
            if step == 1:
                out[f"{tag}/y1"] = y.detach().numpy().copy()
                if tag == "m01":
                    grads(y, xin, "grad_train")
            if step in (1, 3):
                out[f"{tag}/buf{step}/running_mean"] = np.stack([bn.running_mean.numpy() for bn in bns])
                out[f"{tag}/buf{step}/running_var"] = np.stack([bn.running_var.numpy() for bn in bns])
                out[f"{tag}/buf{step}/nbt"] = np.stack([bn.num_batches_tracked.numpy() for bn in bns])
        bns.eval()
        xin = x[0].clone().requires_grad_(True)
        y = star_loop(bns, xin, ids, offset, sw, sb)
        out[f"{tag}/y_eval"] = y.detach().numpy().copy()
        if tag == "m01":
            grads(y, xin, "grad_eval")
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "mdr_bn")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
