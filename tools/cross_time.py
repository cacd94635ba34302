"""Cost of DCN's cross network (csrc/cross.hip) at B = 8192: the vector form with L = 2 (main.py's defaults) at N = 608 (the
AliCCP 19 x 32) and at N = 4096 (the limit), and the matrix form with L = 3 at N = 608, against the same layer as torch ops on
the same GPU - deepctr's tensordot / matmul form under autograd: what a port of DCN runs without these kernels.  That baseline
is not the code under test.  Writes profiles/cross_time.txt, per shape:
  - the library's forward (satrans_cross_fwd) and forward + backward (satrans_cross_fwd then satrans_cross_bwd) on preallocated
    buffers: device events around the calls, so kernels only, no host work between; beside them the roofline - vector: the
    bytes that must move (forward: x0 in, x_L out; with the backward: + dy in, x0 in, dx out) over 6.3 TB/s; matrix: the
    arithmetic (2 B N^2 per layer forward, three times that with the backward's two products) over the 155 TFLOP/s fp32
    matrix peak;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - CrossNet.forward + backward as a user calls it (autograd, allocation of the saved and work buffers included) and the torch
    form, by the host's clock around a device synchronise, in ALTERNATING rounds; median (min, max) over the rounds;
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two results, relative to max|result|.
Each shape runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/cross_time.py [--reps 10] [--inner 3] [--out profiles/cross_time.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8192, 608, 2, 0), (8192, 4096, 2, 0), (8192, 608, 3, 1))      # B, N, L, matrix
PEAK_TFLOPS = 155.0      # fp32 matrix peak of the MI355X
COPY_TBS = 6.3           # measured copy rate
CHILD_LIMIT_S = 200
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def fmt(t, unit="ms"):
    return f"median {t[0]:.4f} {unit} (min {t[1]:.4f}, max {t[2]:.4f})"


def stats(v):
    return median(v), min(v), max(v)


def events_ms(fn, reps, inner):
    import torch
    for _ in range(inner):
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
        out.append(a.elapsed_time(b) / inner)
    return stats(out)


def wall_ms(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def run(B, N_, L, matrix, reps, inner):
    import torch
    from satrans_amd import CrossNet, layers, native as N
    lib = N.lib()
    form = "matrix" if matrix else "vector"
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== {form} form, B = {B}, N = {N_}, L = {L}"]
    torch.manual_seed(B + N_ + L)
    mod = CrossNet(N_, L, form).to(DEV)
    with torch.no_grad():
        mod.bias.normal_(0, 0.3)
    x = torch.randn(B, N_, device=DEV, requires_grad=True)
    up = torch.randn(B, N_, device=DEV)

    def clear():
        mod.zero_grad(set_to_none=True)
        x.grad = None

    def torch_f():      # deepctr's form
        x_0 = x.unsqueeze(2)
        x_l = x_0
        for i in range(L):
            if matrix:
                x_l = x_0 * (torch.matmul(mod.kernels[i], x_l) + mod.bias[i]) + x_l
            else:
                xl_w = torch.tensordot(x_l, mod.kernels[i], dims=([1], [0]))
                x_l = torch.matmul(x_0, xl_w) + mod.bias[i] + x_l
        return torch.squeeze(x_l, dim=2)

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    def mod_fb():
        clear()
        (mod(x) * up).sum().backward()

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        kernels, bias, xd = mod.kernels.detach().contiguous(), mod.bias.detach().contiguous(), x.detach().contiguous()
        d = layers._cross_desc(xd, matrix, kernels, bias)
        saved = torch.empty(int(lib.satrans_cross_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        work = torch.empty(int(lib.satrans_cross_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        result, dx = torch.empty_like(xd), torch.empty_like(xd)
        dk, db = torch.empty_like(kernels), torch.empty_like(bias)
        g = N.CrossGrads()
        g.kernels, g.bias = dk.data_ptr(), db.data_ptr()
    stream = N.stream_handle(torch.device(DEV))

    def lib_f():
        N.check(lib.satrans_cross_fwd(ctypes.byref(d), result.data_ptr(), saved.data_ptr(), stream), "satrans_cross_fwd")

    def lib_fb():
        lib_f()
        N.check(lib.satrans_cross_bwd(ctypes.byref(d), up.data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(), ctypes.byref(g),
                                      stream), "satrans_cross_bwd")

    with torch.no_grad():
        y_new, y_old = mod(x), torch_f()
    lines.append(f"largest |CrossNet - torch form| / max|result|: {float((y_new - y_old).abs().max() / y_old.abs().max()):.2e}")
    mem_new, mem_old = peak_mb(mod_fb), peak_mb(torch_fb)
    k_f, k_fb = events_ms(lib_f, reps, inner), events_ms(lib_fb, reps, inner)
    t_f, t_fb = events_ms(torch_f, reps, inner), events_ms(torch_fb, reps, inner)
    for fn in (mod_fb, torch_fb):
        wall_ms(fn, inner)
    w_new, w_old = [], []
    for _ in range(reps):      # alternating rounds
        w_new.append(wall_ms(mod_fb, inner))
        w_old.append(wall_ms(torch_fb, inner))
    w_new, w_old = stats(w_new), stats(w_old)
    if matrix:
        fl = 2.0 * B * N_ * N_ * L
        roof_f, roof_fb = fl / (PEAK_TFLOPS * 1e12) * 1e3, 3 * fl / (PEAK_TFLOPS * 1e12) * 1e3
        what_f, what_fb = f"{fl / 1e9:.1f} GFLOP", f"{3 * fl / 1e9:.1f} GFLOP"
    else:
        by = 4.0 * B * N_
        roof_f, roof_fb = 2 * by / (COPY_TBS * 1e12) * 1e3, 5 * by / (COPY_TBS * 1e12) * 1e3
        what_f, what_fb = f"{2 * by / 1e6:.1f} MB", f"{5 * by / 1e6:.1f} MB"
    lines.append(f"library forward (device events):             {fmt(k_f)}    roofline {what_f}: {roof_f:.4f} ms, "
                 f"{100 * roof_f / k_f[0]:.1f} % of it")
    lines.append(f"torch form forward (device events):          {fmt(t_f)}    torch / library = {t_f[0] / k_f[0]:.2f}")
    lines.append(f"library forward + backward (device events):  {fmt(k_fb)}    roofline {what_fb}: {roof_fb:.4f} ms, "
                 f"{100 * roof_fb / k_fb[0]:.1f} % of it")
    lines.append(f"torch form forward + backward (events):      {fmt(t_fb)}    torch / library = {t_fb[0] / k_fb[0]:.2f}")
    lines.append(f"CrossNet module forward + backward (host clock): {fmt(w_new)}")
    lines.append(f"torch form forward + backward (host clock):      {fmt(w_old)}    torch / module = {w_old[0] / w_new[0]:.2f}")
    lines.append(f"peak memory above the start, forward + backward: module {mem_new:.1f} MB, torch form {mem_old:.1f} MB    "
                 f"torch / module = {mem_old / mem_new:.1f}")
    lines.append(f"(one [B, N] fp32: {B * N_ * 4 / 1e6:.1f} MB; saved {saved.numel() * 4 / 1e6:.2f} MB, workspace "
                 f"{work.numel() * 4 / 1e6:.2f} MB)")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_time.txt"))
    ap.add_argument("--shape", type=int, nargs=4, default=None, help="(internal) run one shape B N L matrix in this process")
    a = ap.parse_args()
    if a.shape is not None:
        run(*a.shape, a.reps, a.inner)
        return
    text = [f"tools/cross_time.py; median (min, max) of {a.reps} repetitions of {a.inner} calls"]
    for shape in SHAPES:      # a child process per shape, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", *map(str, shape), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"shape {shape}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {shape}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
