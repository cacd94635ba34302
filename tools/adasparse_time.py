"""Cost of AdaSparse's scenario-pruned DNN (csrc/adasparse.hip) at the reference's wiring: B = 8192, C = 608 (19 fields x 32),
E = 32, main.py's widths (256, 128), against the reference's DNN_w_Pruner statement written in plain torch on the same GPU
(tests/adasparse_reference.py::torch_form: per layer a cat, two products and the pointwise chain, autograd for the backward).
That baseline is not the code under test: torch dispatches its products to rocBLAS.  Writes profiles/adasparse_time.txt:
  - AdaSparseHead forward + backward as a user calls it (the sigmoid and the summed BCE, autograd included);
  - the torch form, forward + backward, and the ratio;
  - the forward alone, fused (one launch per layer: both products over one staged row tile, then the epilogue) against
    composed from the existing kernels (satrans_adasparse_set_forward(1): the plain tile product twice, the second over a
    concatenated copy, and a pointwise epilogue), and forward + backward with the composed forward;
  - the largest difference between the module and the torch form on the probabilities, and fused against composed;
  - the multiply-add count per row.
Device events around `--inner` calls, warmed; median, minimum and maximum of `--reps` such boxes.  The shape runs in a child
process of its own under a time limit; nothing starts after a failure.
Usage: python tools/adasparse_time.py [--reps 20] [--inner 5] [--out profiles/adasparse_time.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8192, 608, 32, (256, 128)),)
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


def run(case, reps, inner):
    import torch
    import torch.nn.functional as F
    from satrans_amd import AdaSparseHead, native as N
    from tests import adasparse_reference as R
    B, CN, E, WIDTHS = SHAPES[case]
    lib = N.lib()
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}"]
    g = torch.Generator().manual_seed(case + 1)
    x, e, _, P = R.draw(B, CN, E, WIDTHS, case + 1, rel=0.0)      # (no rows drawn again: nothing here is held to a bound)
    labels = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    x, e = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    mod = AdaSparseHead(CN, WIDTHS, domain_emb_dim=E)
    mod.load_state_dict(R.state_from_params(P))
    mod = mod.to(DEV)
    L = len(WIDTHS)

    def params():
        return R.params_from_state(dict(mod.named_parameters()), L, dtype=torch.float32)

    def clear():
        mod.zero_grad(set_to_none=True)
        x.grad = e.grad = None

    def mod_fb():
        clear()
        F.binary_cross_entropy(torch.sigmoid(mod(x, e)).squeeze(1), labels, reduction='sum').backward()

    def torch_fb():
        clear()
        F.binary_cross_entropy(torch.sigmoid(R.torch_form(x, e, params())).squeeze(1), labels, reduction='sum').backward()

    def mod_f():
        with torch.no_grad():
            return mod(x, e)

    with torch.no_grad():
        p_new = torch.sigmoid(mod(x, e))
        p_old = torch.sigmoid(R.torch_form(x, e, params()))
        shares = [float((pi == 0).float().mean()) for pi in mod.last_pi]
    lines.append(f"== B = {B}, C = {CN}, E = {E}, widths {WIDTHS} (pruned share per layer: " + ", ".join(f"{s:.2f}" for s in shares) + ")")
    lines.append(f"largest |AdaSparseHead - torch form| on a probability: {float((p_new - p_old).abs().max()):.2e}")
    t_fb, l_fb, t_f = events_us(mod_fb, reps, inner), events_us(torch_fb, reps, inner), events_us(mod_f, reps, inner)
    assert lib.satrans_adasparse_set_forward(1) == 0
    try:
        p_comp = torch.sigmoid(mod_f())
        c_f, c_fb = events_us(mod_f, reps, inner), events_us(mod_fb, reps, inner)
    finally:
        lib.satrans_adasparse_set_forward(0)
    lines.append(f"AdaSparseHead forward + backward (module call, fused forward): {fmt(t_fb)}")
    lines.append(f"torch form forward + backward:                                 {fmt(l_fb)}    torch / module = {l_fb[0] / t_fb[0]:.2f}")
    lines.append(f"forward alone, fused (1 launch per layer):                     {fmt(t_f)}")
    lines.append(f"forward alone, composed (4 launches per layer):                {fmt(c_f)}    composed / fused = {c_f[0] / t_f[0]:.2f}")
    lines.append(f"forward + backward with the composed forward:                  {fmt(c_fb)}")
    lines.append(f"largest |fused - composed| on a probability: {float((p_new - p_comp).abs().max()):.2e}")
    units = (CN,) + tuple(WIDTHS)
    macs = sum(k * n + (k + E) * n for k, n in zip(units[:-1], units[1:])) + WIDTHS[-1]
    lines.append(f"multiply-adds per row, forward: {macs} (linears {sum(k * n for k, n in zip(units[:-1], units[1:]))}, pruners "
                 f"{sum((k + E) * n for k, n in zip(units[:-1], units[1:]))}, logit {WIDTHS[-1]}); the backward does twice that")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adasparse_time.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run one shape in this process")
    a = ap.parse_args()
    if a.case is not None:
        run(a.case, a.reps, a.inner)
        return
    text = [f"tools/adasparse_time.py; device events around {a.inner} calls, median (min, max) of {a.reps} repetitions"]
    for case in range(len(SHAPES)):      # a child process per shape, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(case), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"shape {SHAPES[case]}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {SHAPES[case]}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
