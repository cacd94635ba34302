"""Cost of the scenario-routed PLE head (csrc/ple.hip) at the reference's wiring: B = 8192, C = 608 (19 fields x 32), main.py's
widths (one specific and one shared expert of (256, 128), two levels, gate (64,), tower (64,)), at T = 3 and T = 32 tasks,
against the reference's UNROUTED form written in plain torch on the same GPU (tests/ple_reference.py::torch_loop: every task's
experts, gates and towers over every row at both levels, the [B,T] probabilities, then the masked loss of
mtl_basemodel.py:268-269).  That baseline is not the code under test: torch dispatches its products to rocBLAS.  Writes
profiles/ple_time.txt:
  - PLEHead forward + backward as a user calls it (bucketing, the one device-to-host read, the stacking of the parameters,
    the sigmoid and the summed BCE, autograd included);
  - the torch form, forward + backward, and the ratio;
  - the largest difference between the two on each row's own-task probability.
Device events around `--inner` calls, warmed; median, minimum and maximum of `--reps` such boxes.  Every shape runs in a child
process of its own under a time limit; nothing starts after a failure.
Usage: python tools/ple_time.py [--reps 20] [--inner 5] [--out profiles/ple_time.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CN, NS, NSH, LEVELS, EXPERT, GATE, TOWER = 8192, 608, 1, 1, 2, (256, 128), (64,), (64,)
SCENARIOS = (3, 32)
CHILD_LIMIT_S = 240
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def events_us(fn, reps, inner):
    import torch
    for _ in range(2 * inner):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return median(out), min(out), max(out)


def fmt(t):
    return f"median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def run(T, reps, inner):
    import torch
    import torch.nn.functional as F
    from satrans_amd import PLEHead, native as N
    from tests import ple_reference as R
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}"]
    x, _, P = R.draw(B, CN, T, NS, NSH, LEVELS, EXPERT, GATE, TOWER, T)
    g = torch.Generator().manual_seed(T)
    ids = torch.randint(0, T, (B,), generator=g).to(DEV)
    labels = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    x = x.to(DEV).requires_grad_(True)
    mod = PLEHead(CN, T, NSH, NS, LEVELS, EXPERT, GATE, TOWER)
    mod.load_state_dict(R.state_from_params(P), strict=False)      # the parameters that take no part keep their initial values
    mod = mod.to(DEV)
    counts = torch.bincount(ids, minlength=T).tolist()
    lines.append(f"== B = {B}, C = {CN}, ns = {NS}, nsh = {NSH}, levels = {LEVELS}, expert {EXPERT}, gate {GATE}, tower {TOWER}, T = {T} "
                 f"(rows per task: min {min(counts)}, max {max(counts)})")
    nx, ng, nt = len(EXPERT), len(GATE), len(TOWER)

    def stacked():
        return R.params_from_state(dict(mod.named_parameters()), T, NS, NSH, LEVELS, nx, ng, nt, dtype=torch.float32)

    def mod_fb():
        mod.zero_grad(set_to_none=True)
        x.grad = None
        F.binary_cross_entropy(torch.sigmoid(mod(x, ids)).squeeze(1), labels, reduction='sum').backward()

    def loop_fb():
        mod.zero_grad(set_to_none=True)
        x.grad = None
        R.masked_loss(R.torch_loop(x, stacked()), labels, ids).backward()

    with torch.no_grad():
        own_new = torch.sigmoid(mod(x, ids)).squeeze(1)
        own_old = R.torch_loop(x, stacked()).gather(1, ids.unsqueeze(1)).squeeze(1)
    lines.append(f"largest |PLEHead - torch form| on a row's own-task probability: {float((own_new - own_old).abs().max()):.2e}")
    t_fb, l_fb = events_us(mod_fb, reps, inner), events_us(loop_fb, reps, inner)
    lines.append(f"PLEHead forward + backward (module call, routed):  {fmt(t_fb)}")
    lines.append(f"torch unrouted form forward + backward:            {fmt(l_fb)}    torch / module = {l_fb[0] / t_fb[0]:.2f}")
    widths = lambda n_in, units, fin: sum(a * b for a, b in zip((n_in,) + tuple(units), tuple(units) + (fin,)))      # noqa: E731
    n = EXPERT[-1]
    x0, x1 = widths(CN, EXPERT[:-1], n), widths(n, EXPERT[:-1], n)      # one expert over x / over a mixture
    g0, g1, tw = widths(CN, GATE, 1) - GATE[-1], widths(n, GATE, 1) - GATE[-1], widths(n, TOWER, 1)      # gate DNNs without their final layer
    Eo, E0 = NS + NSH, T * NS + NSH
    unrouted = E0 * x0 + T * (g0 + GATE[-1] * Eo) + g0 + GATE[-1] * E0 + E0 * x1 + T * (g1 + GATE[-1] * Eo) + T * tw
    routed = E0 * x0 + (g0 + GATE[-1] * Eo) + g0 + GATE[-1] * E0 + Eo * x1 + (g1 + GATE[-1] * Eo) + tw
    lines.append(f"multiply-adds per row: level-0 experts {E0 * x0} (both forms); the unrouted form does {unrouted} in all, the "
                 f"routed one {routed} ({unrouted / routed:.2f}x fewer)")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ple_time.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run one T in this process")
    a = ap.parse_args()
    if a.case is not None:
        run(a.case, a.reps, a.inner)
        return
    text = [f"tools/ple_time.py; device events around {a.inner} calls, median (min, max) of {a.reps} repetitions"]
    for T in SCENARIOS:      # a child process per shape, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(T), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"T = {T}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"T = {T}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
