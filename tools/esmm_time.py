"""Cost of ESMMHead and WDLHead (csrc/esmm.hip) at B = 8192, C = 608 (19 fields x 32), towers / hidden units (256, 128):
forward + backward as a user calls it (the module, the summed BCE over its output, autograd), per head in three forms:
  (a) the head with the fused tail (one launch: the last hidden layer, the final layer, and for ESMM the sigmoids and the product);
  (b) the head composed from the shared tile product (satrans_esmm_set_forward(1): two launches of the product, the second with
      one output column, and for ESMM a pointwise kernel);
  (c) the literal torch form on the same GPU (Linear, relu, F.dropout, sigmoid, product; autograd for the backward).  That
      baseline is not the code under test: torch dispatches its products to rocBLAS.
(a), (b) and (c) without dropout (training mode, p = 0) and at dnn_dropout = 0.5.  Also: the largest difference between the head
and the torch form without dropout, fused - composed (must print 0), and the decision the measurement is for: the fused tail is
the default only if (a)'s median is below (b)'s by more than (b)'s own min-max spread.  It is not, so the library ships (b).
Device events around `--inner` calls, warmed; median, minimum and maximum of `--reps` such boxes, the six forms of a head timed
in turn inside every repetition (two earlier runs that timed them one after the other disagreed by 20 % on the same code).  Each head runs in a child
process of its own under a time limit; nothing starts after a failure.  Writes profiles/esmm_time.txt; `--note TEXT` records a
line with the measurements (what else was checked on the same build).
Usage: python tools/esmm_time.py [--reps 30] [--inner 10] [--out profiles/esmm_time.txt] [--note TEXT]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CN, HIDDEN = 8192, 608, (256, 128)
HEADS = ((2, "ESMMHead"), (1, "WDLHead"))
CHILD_LIMIT_S = 240
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternating_us(fns, reps, inner):
    """{name: (median, min, max)} of the functions `fns`, timed in turn: every repetition times one box of `inner` calls of
    each, so that a drift of the machine falls on all of them alike."""
    import torch
    for fn in fns.values():
        for _ in range(2 * inner):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: (median(v), min(v), max(v)) for k, v in out.items()}


def fmt(t):
    return f"median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def run(case, reps, inner):
    import torch
    import torch.nn.functional as F
    from satrans_amd import ESMMHead, WDLHead, native as N
    from tests import esmm_reference as R
    towers, name = HEADS[case]
    lib = N.lib()
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}"]
    g = torch.Generator().manual_seed(case + 1)
    x = torch.randn(B, CN, generator=g).to(DEV).requires_grad_(True)
    labels = (torch.rand(B, towers, generator=g) > 0.5).float().to(DEV)
    heads = {}
    for p in (0.0, 0.5):
        torch.manual_seed(3)      # the same initial draws for both
        heads[p] = (ESMMHead if towers == 2 else WDLHead)(CN, HIDDEN, init_std=CN ** -0.5, dnn_dropout=p).to(DEV).train()

    def clear(mod):
        mod.zero_grad(set_to_none=True)
        x.grad = None

    def prob(y):
        return y if towers == 2 else torch.sigmoid(y)

    def head_fb(p, composed):
        def fn():
            lib.satrans_esmm_set_forward(composed)
            clear(heads[p])
            F.binary_cross_entropy(prob(heads[p](x)), labels, reduction='sum').backward()
        return fn

    def literal(mod, p):
        outs = []
        for dnn, final in zip(R.dnn_names(towers), R.final_names(towers)):
            h = x
            for lin in getattr(mod, dnn).linears:
                h = F.dropout(F.relu(lin(h)), p, training=True)
            outs.append(getattr(mod, final)(h) + mod.out.bias)
        if towers == 1:
            return outs[0]
        ctr, cvr = torch.sigmoid(outs[0]), torch.sigmoid(outs[1])
        return torch.cat([ctr, ctr * cvr], -1)

    def torch_fb(p):
        def fn():
            clear(heads[p])
            F.binary_cross_entropy(prob(literal(heads[p], p)), labels, reduction='sum').backward()
        return fn

    lines.append(f"== {name}: B = {B}, C = {CN}, hidden units {HIDDEN}, {towers} tower(s)")
    with torch.no_grad():
        y_new, y_old = heads[0.0](x), literal(heads[0.0], 0.0)
    lines.append(f"largest |{name} - torch form| on its output, no dropout: {float((y_new - y_old).abs().max()):.2e}")
    default = lib.satrans_esmm_set_forward(0)
    try:
        with torch.no_grad():
            y_new = heads[0.0](x)
        lib.satrans_esmm_set_forward(1)
        with torch.no_grad():
            y_comp = heads[0.0](x)
        fns = {}
        for p in (0.0, 0.5):
            fns.update({("a", p): head_fb(p, 0), ("b", p): head_fb(p, 1), ("c", p): torch_fb(p)})
        t = alternating_us(fns, reps, inner)
        fused, composed, plain = ({p: t[(k, p)] for p in (0.0, 0.5)} for k in "abc")
    finally:
        lib.satrans_esmm_set_forward(default)
    lines.append(f"the library's default form: {'composed' if default else 'fused tail'}")
    for p in (0.0, 0.5):
        a, b, c = fused[p], composed[p], plain[p]
        lines.append(f"dnn_dropout = {p}, forward + backward (module call, summed BCE, autograd):")
        lines.append(f"  (a) fused tail:        {fmt(a)}")
        lines.append(f"  (b) composed:          {fmt(b)}    (b) / (a) = {b[0] / a[0]:.3f}")
        lines.append(f"  (c) literal torch:     {fmt(c)}    (c) / (a) = {c[0] / a[0]:.3f}")
        lines.append(f"  (a) faster than (b) by more than (b)'s spread ({b[0] - a[0]:.1f} us against {b[2] - b[1]:.1f} us): "
                     f"{b[0] - a[0] > b[2] - b[1]}")
    lines.append(f"dropout 0.5 against 0, fused: {fused[0.5][0] / fused[0.0][0]:.3f}; literal torch: {plain[0.5][0] / plain[0.0][0]:.3f}")
    lines.append(f"fused - composed, largest difference on the output: {float((y_new - y_comp).abs().max()):g}")
    chain = sum(k * n for k, n in zip((CN,) + HIDDEN[:-1], HIDDEN)) + HIDDEN[-1]
    lines.append(f"multiply-adds per row, forward: {towers * chain} ({towers} x {chain}); the backward does twice that")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esmm_time.txt"))
    ap.add_argument("--note", default=None, help="a line recorded with the measurements")
    ap.add_argument("--case", type=int, default=None, help="(internal) run one head in this process")
    a = ap.parse_args()
    if a.case is not None:
        run(a.case, a.reps, a.inner)
        return
    text = [f"tools/esmm_time.py; device events around {a.inner} calls, median (min, max) of {a.reps} repetitions, the forms in turn"]
    for case in range(len(HEADS)):      # a child process per head, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(case), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{HEADS[case][1]}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{HEADS[case][1]}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    if a.note:
        text.append(a.note)
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
