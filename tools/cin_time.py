"""Cost of the compressed interaction network (csrc/cin.hip) at the AliCCP shape of the reference's xDeepFM: F = 19 fields,
D = 32, cin_layer_size (256, 128), split_half, at B = 4096 (the batch main.py gives xDeepFM) and 8192, against the same CIN as
torch ops on the same GPU - the einsum over the fields, the reshape to [B, H M, D] and F.conv1d, under autograd: what a port
of xDeepFM runs without these kernels.  That baseline is not the code under test: torch dispatches its products to its BLAS
and convolution libraries.  Writes profiles/cin_time.txt, per B:
  - the library's forward (satrans_cin_fwd: one launch per layer and the sum over d) and forward + backward (satrans_cin_fwd
    then satrans_cin_bwd) on preallocated buffers: device events around the calls, so kernels only, no host work between;
    the arithmetic these need (2 B D sum_i O_i H_i M flops forward, three times that with the backward's two products) over
    that time as a share of the 155 TFLOP/s fp32 matrix peak;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - CIN.forward + backward as a user calls it (autograd, allocation of the saved and work buffers included) and the torch
    form, by the host's clock around a device synchronise, in ALTERNATING rounds; median (min, max) over the rounds;
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two results, relative to max|result|.
Each shape runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/cin_time.py [--reps 10] [--inner 3] [--out profiles/cin_time.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, D, LAYERS, SPLIT = 19, 32, (256, 128), True
BATCHES = (4096, 8192)
PEAK_TFLOPS = 155.0      # fp32 matrix peak of the MI355X
CHILD_LIMIT_S = 300
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def fmt(t, unit="ms"):
    return f"median {t[0]:.3f} {unit} (min {t[1]:.3f}, max {t[2]:.3f})"


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


def flops_forward(B):
    total, h = 0, M
    for i, o in enumerate(LAYERS):
        total += 2 * B * D * o * h * M
        h = o // 2 if SPLIT and i != len(LAYERS) - 1 else o
    return total


def run(B, reps, inner):
    import torch
    import torch.nn.functional as F
    from satrans_amd import CIN, layers, native as N
    lib = N.lib()
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== B = {B}, M = {M}, D = {D}, layers {LAYERS}, split_half {SPLIT}"]
    torch.manual_seed(B)
    mod = CIN(M, LAYERS, split_half=SPLIT).to(DEV)
    x = torch.randn(B, M, D, device=DEV, requires_grad=True)
    up = torch.randn(B, mod.featuremap_num, device=DEV)

    def clear():
        mod.zero_grad(set_to_none=True)
        x.grad = None

    def torch_f():
        hidden, final = x, []
        for i, conv in enumerate(mod.conv1ds):
            z = torch.einsum('bhd,bmd->bhmd', hidden, x).reshape(B, hidden.shape[1] * M, D)
            z = torch.relu(F.conv1d(z, conv.weight, conv.bias))
            if SPLIT and i != len(LAYERS) - 1:
                hidden, direct = torch.split(z, 2 * [LAYERS[i] // 2], 1)
            else:
                hidden = direct = z
            final.append(direct)
        return torch.cat(final, dim=1).sum(-1)

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    def mod_fb():
        clear()
        (mod(x) * up).sum().backward()

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        tensors = [c.weight.detach().contiguous() for c in mod.conv1ds] + [c.bias.detach().contiguous() for c in mod.conv1ds]
        xd = x.detach().contiguous()
        d = layers._cin_desc(xd, SPLIT, tensors)
        saved = torch.empty(int(lib.satrans_cin_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        work = torch.empty(int(lib.satrans_cin_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        result, dx = torch.empty_like(up), torch.empty_like(xd)
        grads = [torch.empty_like(t) for t in tensors]
        g = layers._cin_fill(N.CINGrads(), len(LAYERS), grads)
    stream = N.stream_handle(torch.device(DEV))

    def lib_f():
        N.check(lib.satrans_cin_fwd(ctypes.byref(d), result.data_ptr(), saved.data_ptr(), stream), "satrans_cin_fwd")

    def lib_fb():
        lib_f()
        N.check(lib.satrans_cin_bwd(ctypes.byref(d), up.data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(), ctypes.byref(g),
                                    stream), "satrans_cin_bwd")

    with torch.no_grad():
        y_new, y_old = mod(x), torch_f()
    lines.append(f"largest |CIN - torch form| / max|result|: {float((y_new - y_old).abs().max() / y_old.abs().max()):.2e}")
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
    fl = flops_forward(B)
    share = lambda flops, ms: 100.0 * flops / (ms * 1e-3) / (PEAK_TFLOPS * 1e12)      # noqa: E731
    lines.append(f"library forward (device events):             {fmt(k_f)}    {fl / 1e9:.1f} GFLOP, {share(fl, k_f[0]):.1f} % of the fp32 matrix peak")
    lines.append(f"torch form forward (device events):          {fmt(t_f)}    torch / library = {t_f[0] / k_f[0]:.2f}")
    lines.append(f"library forward + backward (device events):  {fmt(k_fb)}    {3 * fl / 1e9:.1f} GFLOP, {share(3 * fl, k_fb[0]):.1f} % of the fp32 matrix peak")
    lines.append(f"torch form forward + backward (events):      {fmt(t_fb)}    torch / library = {t_fb[0] / k_fb[0]:.2f}")
    lines.append(f"CIN module forward + backward (host clock):  {fmt(w_new)}")
    lines.append(f"torch form forward + backward (host clock):  {fmt(w_old)}    torch / module = {w_old[0] / w_new[0]:.2f}")
    lines.append(f"peak memory above the start, forward + backward: module {mem_new:.1f} MB, torch form {mem_old:.1f} MB    "
                 f"torch / module = {mem_old / mem_new:.1f}")
    lines.append(f"(layer 2's outer product alone, [B, {LAYERS[0] // 2 * M}, {D}] fp32: {B * (LAYERS[0] // 2) * M * D * 4 / 1e6:.1f} MB; "
                 f"saved activations {saved.numel() * 4 / 1e6:.1f} MB, workspace {work.numel() * 4 / 1e6:.1f} MB)")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cin_time.txt"))
    ap.add_argument("--batch", type=int, default=None, help="(internal) run one batch size in this process")
    a = ap.parse_args()
    if a.batch is not None:
        run(a.batch, a.reps, a.inner)
        return
    text = [f"tools/cin_time.py; median (min, max) of {a.reps} repetitions of {a.inner} calls"]
    for B in BATCHES:      # a child process per shape, each under its own time limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"B = {B}: no result within {CHILD_LIMIT_S} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"B = {B}: exit status {r.returncode}; stopping")
        text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
