"""Cost of STAR's star-topology towers (csrc/star.hip) at the reference's wiring: B = 8192, C = 608 (19 fields x 32), hidden
(256, 128), at S = 3 and S = 32, against the reference's form on the same GPU - the loop of models/star.py:147-170 as torch
ops: two boolean-mask selects, the elementwise weight products and bias sums, F.linear, relu, masked write-back, per scenario.
Writes profiles/star_time.txt:
  - StarTowers forward + backward as a user calls it (bucketing, the one device-to-host read, the stacking of the per-scenario
    parameters and autograd included);
  - the launches of satrans_star_fwd / satrans_star_bwd alone, their FLOPs as a fraction of the fp32-MFMA rate this project
    measured (155 TFLOP/s, profiles/r05_valu_rates.txt) and their compulsory HBM bytes;
  - the torch loop, forward + backward, and the ratio.
Device events around `--inner` calls, warmed, median of `--reps` repetitions.  Every shape runs in a child process of its own
under a time limit; nothing starts after a failure.
Usage: python tools/star_time.py [--reps 20] [--inner 5] [--out profiles/star_time.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CN, HIDDEN = 8192, 608, (256, 128)
SCENARIOS = (3, 32)
MFMA_F32_TFLOPS = 155.0
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


def torch_loop(mod, x, ids):
    import torch
    import torch.nn.functional as F
    logit = torch.zeros(x.shape[0], 1, device=x.device)
    for s in range(mod.num_domains):
        h = x[ids == s]
        for l, shared in enumerate(mod.shared_dnn.linears):
            own = mod.domain_dnns[s].linears[l]
            h = torch.relu(F.linear(h, own.weight * shared.weight, own.bias + shared.bias))
        own = mod.domain_dnn_linears[s]
        logit[ids == s] = F.linear(h, own.weight * mod.shared_dnn_linear.weight, own.bias + mod.shared_dnn_linear.bias)
    return logit


def run(S, reps, inner):
    import torch
    from satrans_amd import StarTowers, native as N
    from satrans_amd.layers import _bucket_rows, _star_desc
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}"]
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, CN, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(B, 1, generator=g).to(DEV)
    ids = torch.randint(0, S, (B,), generator=g).to(DEV)
    mod = StarTowers(CN, HIDDEN, S, init_std=CN ** -0.25).to(DEV)
    counts = torch.bincount(ids, minlength=S).tolist()
    lines.append(f"== B = {B}, C = {CN}, hidden = {HIDDEN}, S = {S} (rows per scenario: min {min(counts)}, max {max(counts)})")

    def mod_fb():
        mod.zero_grad(set_to_none=True)
        (mod(x, ids) * w).sum().backward()

    def loop_fb():
        mod.zero_grad(set_to_none=True)
        (torch_loop(mod, x, ids) * w).sum().backward()

    y_new, y_old = mod(x, ids), torch_loop(mod, x, ids)
    lines.append(f"largest |StarTowers - torch loop| on these rows: {float((y_new - y_old).abs().max()):.2e} "
                 f"(largest |logit| {float(y_old.abs().max()):.2e})")
    t_fb, l_fb = events_us(mod_fb, reps, inner), events_us(loop_fb, reps, inner)
    lines.append(f"StarTowers forward + backward (module call): {fmt(t_fb)}")
    lines.append(f"torch loop forward + backward:               {fmt(l_fb)}    loop / module = {l_fb[0] / t_fb[0]:.2f}")

    # the launches alone
    lib = N.lib()
    st = N.stream_handle(torch.device(DEV))
    xd = x.detach()
    order, seg, _ = _bucket_rows(xd, ids, S, 0, "star_time")
    L = len(HIDDEN) + 1
    doms = [[mod.domain_dnns[s].linears[l] for s in range(S)] for l in range(L - 1)] + [list(mod.domain_dnn_linears)]
    shared = list(mod.shared_dnn.linears) + [mod.shared_dnn_linear]
    tensors = [torch.stack([m.weight.detach() for m in layer]) for layer in doms] + \
              [torch.stack([m.bias.detach() for m in layer]) for layer in doms] + \
              [m.weight.detach() for m in shared] + [m.bias.detach() for m in shared]
    d = _star_desc(xd, order, seg, L, tensors)
    saved = torch.empty(int(lib.satrans_star_saved_floats(C.byref(d))), device=DEV)
    work = torch.empty(int(lib.satrans_star_workspace_floats(C.byref(d))), device=DEV)
    logit, dx = torch.empty(B, 1, device=DEV), torch.empty_like(xd)
    grads = [torch.empty_like(t) for t in tensors]
    groups = [(C.c_void_p * L)(*[t.data_ptr() for t in grads[k * L:(k + 1) * L]]) for k in range(4)]

    def k_fwd():
        N.check(lib.satrans_star_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), st), "fwd")

    def k_both():
        k_fwd()
        N.check(lib.satrans_star_bwd(C.byref(d), w.data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(), groups[0], groups[1],
                                     groups[2], groups[3], st), "bwd")

    k_f, k_fb = events_us(k_fwd, reps, inner), events_us(k_both, reps, inner)
    widths = [CN] + list(HIDDEN) + [1]
    macs = sum(widths[i] * widths[i + 1] for i in range(L))
    params = 4 * (S + 1) * sum(widths[i + 1] * (widths[i] + 1) for i in range(L))
    rows, hid = 4 * B * CN, 4 * B * sum(HIDDEN)
    for name, t, flop, nbytes, what in (
            (f"satrans_star_fwd ({L} launches)", k_f, 2 * B * macs, rows + hid + params, "x and parameters read, hidden rows written"),
            (f"satrans_star_fwd + _bwd ({4 * L} launches)", k_fb, 6 * B * macs, 3 * rows + 2 * hid + 3 * params,
             "x read twice, dx written, hidden rows written and read, parameters read twice, their gradients written")):
        tf = flop / t[0] / 1e6
        lines.append(f"{name}: {fmt(t)}; {flop / 1e9:.2f} GFLOP = {tf:.1f} TFLOP/s = {tf / MFMA_F32_TFLOPS:.3f} of the "
                     f"{MFMA_F32_TFLOPS:.0f} TFLOP/s fp32-MFMA rate (matrix time {flop / MFMA_F32_TFLOPS / 1e6:.1f} us); "
                     f"compulsory HBM bytes {nbytes / 1e6:.1f} MB ({what}); workspace {work.numel() * 4 / 1e6:.1f} MB")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_time.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run one S in this process")
    a = ap.parse_args()
    if a.case is not None:
        run(a.case, a.reps, a.inner)
        return
    text = [f"tools/star_time.py; device events around {a.inner} calls, median of {a.reps} repetitions"]
    for S in SCENARIOS:      # a child process per shape, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(S), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"S = {S}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"S = {S}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
