"""Cost of the scenario-routed SharedBottom head (csrc/sharedbottom.hip) at the reference's wiring: B = 8192, C = 608 (19
fields x 32), main.py's widths bottom (256, 128), tower (64,), for T = 3 and T = 32 tasks with random ids, against the
reference's unrouted form written in plain torch on the same GPU (tests/sharedbottom_reference.py::torch_loop: every task's
tower over every row, one column read per row, autograd for the backward).  That baseline is not the code under test: torch
dispatches its products to rocBLAS.  Writes profiles/sharedbottom_time.txt, per T:
  - SharedBottomHead forward + backward as a user calls it (bucketing, the sigmoid and the summed BCE, autograd included);
  - the torch unrouted form, forward + backward, and the ratio;
  - the forward alone, with the fused tower tail (one launch: the last tower layer, the final layer and the out bias) and
    composed from the shared tile product (satrans_sharedbottom_set_forward(1): two launches, the second with one output
    column): the library call on a bucketed batch (device work only) and the module call under no_grad (bucketing and its
    device-to-host read included);
  - forward + backward with the composed forward;
  - the largest difference between the module and the torch form on a probability, and fused - composed (must print 0);
  - the multiply-add count per row, routed and unrouted.
Device events around `--inner` calls, warmed; median, minimum and maximum of `--reps` such boxes.  Each shape runs in a child
process of its own under a time limit; nothing starts after a failure.
Usage: python tools/sharedbottom_time.py [--reps 20] [--inner 5] [--out profiles/sharedbottom_time.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8192, 608, 3, (256, 128), (64,)), (8192, 608, 32, (256, 128), (64,)))
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
    from satrans_amd import SharedBottomHead, layers, native as N
    from tests import sharedbottom_reference as R
    B, CN, T, BOTTOM, TOWER = SHAPES[case]
    lib = N.lib()
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}"]
    g = torch.Generator().manual_seed(case + 1)
    x, _, P = R.draw(B, CN, T, BOTTOM, TOWER, case + 1)      # (no rows drawn again: nothing here is held to a bound)
    ids = torch.randint(0, T, (B,), generator=g).to(DEV)
    labels = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    x = x.to(DEV).requires_grad_(True)
    mod = SharedBottomHead(CN, T, BOTTOM, TOWER)
    mod.load_state_dict(R.state_from_params(P))
    mod = mod.to(DEV)
    nb, nt = len(BOTTOM), len(TOWER)
    col = ids.unsqueeze(1)

    def params():
        return R.params_from_state(dict(mod.named_parameters()), T, nb, nt, dtype=torch.float32)

    def clear():
        mod.zero_grad(set_to_none=True)
        x.grad = None

    def mod_fb():
        clear()
        F.binary_cross_entropy(torch.sigmoid(mod(x, ids)).squeeze(1), labels, reduction='sum').backward()

    def torch_fb():
        clear()
        y = R.torch_loop(x, params()).gather(1, col)
        F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum').backward()

    def mod_f():
        with torch.no_grad():
            return mod(x, ids)

    # the library's forward alone, on a bucketed batch: what the two forms of the tail differ in, without the host's share
    with torch.no_grad():
        order, seg, _ = layers._bucket_rows(x, ids, T, 0, "sharedbottom_time")
        Pd = params()
        tensors = [t.contiguous() for t in Pd["bottom_w"] + Pd["bottom_b"] + Pd["tower_w"] + Pd["tower_b"]] + \
            [Pd["tower_final_w"].contiguous(), Pd["out_bias"].contiguous()]
        xd = x.detach().contiguous()
        d = layers._sharedbottom_desc(xd, order, seg, (nb, nt), tensors)
        saved = torch.empty(int(lib.satrans_sharedbottom_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        logit = torch.empty(B, dtype=torch.float32, device=DEV)
    stream = N.stream_handle(torch.device(DEV))

    def lib_f():
        N.check(lib.satrans_sharedbottom_fwd(ctypes.byref(d), logit.data_ptr(), saved.data_ptr(), stream), "satrans_sharedbottom_fwd")

    with torch.no_grad():
        p_new = torch.sigmoid(mod(x, ids))
        p_old = R.torch_loop(x, params()).gather(1, col)
    lines.append(f"== B = {B}, C = {CN}, T = {T}, bottom {BOTTOM}, tower {TOWER}")
    lines.append(f"largest |SharedBottomHead - torch form| on a probability: {float((p_new - p_old).abs().max()):.2e}")
    assert lib.satrans_sharedbottom_set_forward(0) == 0
    t_fb, l_fb = events_us(mod_fb, reps, inner), events_us(torch_fb, reps, inner)
    t_lf, t_f = events_us(lib_f, reps, inner), events_us(mod_f, reps, inner)
    assert lib.satrans_sharedbottom_set_forward(1) == 0
    try:
        p_comp = torch.sigmoid(mod_f())
        c_lf, c_f, c_fb = events_us(lib_f, reps, inner), events_us(mod_f, reps, inner), events_us(mod_fb, reps, inner)
    finally:
        lib.satrans_sharedbottom_set_forward(0)
    lines.append(f"SharedBottomHead forward + backward (module call, fused tail): {fmt(t_fb)}")
    lines.append(f"torch unrouted form forward + backward:                        {fmt(l_fb)}    torch / module = {l_fb[0] / t_fb[0]:.2f}")
    lines.append(f"forward alone, library call, fused tail ({nb + nt} launches):         {fmt(t_lf)}")
    lines.append(f"forward alone, library call, composed ({nb + nt + 1} launches):          {fmt(c_lf)}    composed / fused = {c_lf[0] / t_lf[0]:.2f}")
    lines.append(f"forward alone, module call, fused tail:                        {fmt(t_f)}")
    lines.append(f"forward alone, module call, composed:                          {fmt(c_f)}    composed / fused = {c_f[0] / t_f[0]:.2f}")
    lines.append(f"forward + backward with the composed forward:                  {fmt(c_fb)}")
    lines.append(f"fused tail's forward median below the composed form's minimum: library call {t_lf[0] < c_lf[1]}, module call {t_f[0] < c_f[1]}")
    lines.append(f"fused - composed, largest difference on a probability: {float((p_new - p_comp).abs().max()):g}")
    chain = lambda units: sum(k * n for k, n in zip(units[:-1], units[1:]))      # noqa: E731
    bottom, tower = chain((CN,) + BOTTOM), chain((BOTTOM[-1],) + TOWER) + (TOWER[-1] if TOWER else BOTTOM[-1])
    lines.append(f"multiply-adds per row, forward: routed {bottom + tower} (bottom {bottom}, one tower {tower}), unrouted "
                 f"{bottom + T * tower} (bottom {bottom}, {T} towers {T * tower}); the backward does twice that")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharedbottom_time.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run one shape in this process")
    a = ap.parse_args()
    if a.case is not None:
        run(a.case, a.reps, a.inner)
        return
    text = [f"tools/sharedbottom_time.py; device events around {a.inner} calls, median (min, max) of {a.reps} repetitions"]
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
