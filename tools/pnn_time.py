"""Cost of the PNN head (csrc/pnn.hip) at the AliCCP shape - F = 19 fields, D = 32, dnn_hidden_units (128, 128): P = 171 pairs - at
B = 4096 and B = 8192, in three configurations: use_inner only, use_outter 'mat' only, and both with 'mat'; against the same head
written as torch ops on the same GPU, fp32: deepctr's literal form (tests/pnn_reference.py: the two gathered [B, P, D] tensors,
for 'mat' the [B, D, P, D] product), a torch DNN, autograd - what a port of PNN runs without these kernels.  That baseline is not
the code under test.
Writes profiles/pnn_time.txt, per batch size and configuration:
  - the library's forward (satrans_pnn_fwd) and forward + backward (then satrans_pnn_bwd) on preallocated buffers: device events
    around the calls, so kernels only, no host work between;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - PNNHead forward + backward as a user calls it (autograd, allocation of the saved and work buffers included) and the torch
    form, by the host's clock around a device synchronise;
    all legs in ALTERNATING rounds, library then torch; median (min - max) over the rounds;
  - every launch of one library forward + backward in launch order with its own duration (torch.profiler's device records,
    median over the profiled calls); from them the share of the fp32 matrix peak that the three 'mat' kernels reach
    (2 P D^2 B FLOP each; the input gradient twice that);
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two logits, relative to max|logit|.
Each (batch size, configuration) runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/pnn_time.py [--reps 10] [--inner 3] [--out profiles/pnn_time.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F_, D_, DNN = 19, 32, (128, 128)
BATCHES = (4096, 8192)
CONFIGS = {"inner": (True, False, "mat"), "mat": (False, True, "mat"), "both": (True, True, "mat")}
PEAK_TFLOPS = 157.3      # fp32 matrix peak of the MI355X
CHILD_LIMIT_S = 240
DEV = "cuda:0"


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def fmt(t, unit="ms"):
    return f"median {t[0]:.4f} {unit} ({t[1]:.4f} - {t[2]:.4f})"


def disjoint(lo, hi):
    return "ranges disjoint" if lo[2] < hi[1] else "ranges OVERLAP"


def event_ms(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


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


def launches(fn, calls):
    """[(kernel name, median us)] of the launches of one fn() in launch order, or None when the device records are missing."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "kernel" in e.name]
        evs.sort(key=lambda e: e.time_range.start)
    except Exception as e:      # (a profiler without device records must not lose the timings above)
        print(f"(per-launch durations unavailable: {type(e).__name__}: {e})")
        return None
    if not evs or len(evs) % calls:
        print(f"(per-launch durations unavailable: {len(evs)} device records for {calls} calls)")
        return None
    per = len(evs) // calls
    out = []
    for i in range(per):
        name = re.search(r"(\w+_kernel)", evs[i].name)
        out.append((name.group(1) if name else evs[i].name[:40], stats([evs[c * per + i].device_time for c in range(calls)])[0]))
    return out


def run(B, config, reps, inner):
    import torch
    from satrans_amd import PNNHead, layers, native as N
    from tests import pnn_reference as R
    lib = N.lib()
    use_inner, use_outter, kind = cfg = CONFIGS[config]
    P = F_ * (F_ - 1) // 2
    n_in = F_ * D_ + P * (int(use_inner) + int(use_outter))
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== B = {B}, '{config}': use_inner {use_inner}, use_outter {use_outter} ('{kind}'), F = {F_}, D = {D_}, dnn {DNN}: "
             f"P = {P}, DNN input {n_in} columns"]
    torch.manual_seed(B)
    head = PNNHead(F_, D_, 0, DNN, use_inner, use_outter, kind, init_std=n_in ** -0.5).to(DEV)
    emb = torch.randn(B, F_, D_, device=DEV, requires_grad=True)
    up = torch.randn(B, 1, device=DEV)

    def clear():
        head.zero_grad(set_to_none=True)
        emb.grad = None

    def torch_f():      # deepctr's literal form over the head's own parameters
        Pm = R.params_from_state(dict(head.named_parameters()), torch.float32)
        return R.forward(emb, None, Pm, cfg)[0]

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    def mod_fb():
        clear()
        (head(emb) * up).sum().backward()

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        kernel = head.outterproduct.kernel.detach() if use_outter else None
        dnn = [l.weight.detach() for l in head.dnn.linears] + [l.bias.detach() for l in head.dnn.linears]
        lin_w, out_b = head.dnn_linear.weight.detach(), head.out.bias.detach()
        xd = emb.detach().contiguous()
        d = layers._pnn_desc(xd, None, (int(use_inner), int(use_outter), N.PNN_KERNEL_TYPES[kind]), kernel, dnn, lin_w, out_b)
        saved = torch.empty(int(lib.satrans_pnn_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        work = torch.empty(int(lib.satrans_pnn_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        logit, demb = torch.empty(B, 1, device=DEV), torch.empty_like(xd)
        gk = None if kernel is None else torch.empty_like(kernel)
        gd, gl, gb = [torch.empty_like(t) for t in dnn], torch.empty_like(lin_w), torch.empty_like(out_b)
        g = layers._pnn_fill(N.PNNGrads(), len(DNN), gk, gd, gl, gb)
    stream = N.stream_handle(torch.device(DEV))

    def lib_f():
        N.check(lib.satrans_pnn_fwd(ctypes.byref(d), logit.data_ptr(), saved.data_ptr(), stream), "satrans_pnn_fwd")

    def lib_fb():
        lib_f()
        N.check(lib.satrans_pnn_bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), None, saved.data_ptr(), work.data_ptr(),
                                    ctypes.byref(g), stream), "satrans_pnn_bwd")

    with torch.no_grad():
        y_new, y_old = head(emb), torch_f()
    lines.append(f"largest |PNNHead - torch form| / max|logit|: {float((y_new - y_old).abs().max() / y_old.abs().max()):.2e}")
    mem_new, mem_old = peak_mb(mod_fb), peak_mb(torch_fb)
    legs = {"k_f": lib_f, "t_f": torch_f, "k_fb": lib_fb, "t_fb": torch_fb}
    for fn in (*legs.values(), mod_fb):      # warm-up
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in (*legs, "w_new", "w_old")}
    for _ in range(reps):      # alternating rounds: library, torch, library, torch, ..
        for k, fn in legs.items():
            got[k].append(event_ms(fn, inner))
        got["w_new"].append(wall_ms(mod_fb, inner))
        got["w_old"].append(wall_ms(torch_fb, inner))
    s = {k: stats(v) for k, v in got.items()}
    lines.append(f"library forward (device events):                    {fmt(s['k_f'])}")
    lines.append(f"torch form forward (device events):                 {fmt(s['t_f'])}    torch / library = "
                 f"{s['t_f'][0] / s['k_f'][0]:.2f}, {disjoint(s['k_f'], s['t_f'])}")
    lines.append(f"library forward + backward (device events):         {fmt(s['k_fb'])}")
    lines.append(f"torch form forward + backward (device events):      {fmt(s['t_fb'])}    torch / library = "
                 f"{s['t_fb'][0] / s['k_fb'][0]:.2f}, {disjoint(s['k_fb'], s['t_fb'])}")
    lines.append(f"PNNHead module forward + backward (host clock):     {fmt(s['w_new'])}")
    lines.append(f"torch form forward + backward (host clock):         {fmt(s['w_old'])}    torch / module = "
                 f"{s['w_old'][0] / s['w_new'][0]:.2f}, {disjoint(s['w_new'], s['w_old'])}")
    lines.append(f"peak memory above the start, forward + backward: module {mem_new:.1f} MB, torch form {mem_old:.1f} MB    "
                 f"torch / module = {mem_old / mem_new:.1f}")
    lines.append(f"(DNN input [B, {n_in}] fp32: {B * n_in * 4 / 1e6:.1f} MB; saved {saved.numel() * 4 / 1e6:.1f} MB, workspace "
                 f"{work.numel() * 4 / 1e6:.1f} MB)")
    print("\n".join(lines), flush=True)
    per = launches(lib_fb, 5)
    if per:
        total = sum(us for _, us in per)
        print(f"launches of one library forward + backward, in launch order (median us of 5 profiled calls; sum {total:.1f} us):")
        for i, (name, us) in enumerate(per):
            print(f"  {i:2d}  {name:28s} {us:9.1f}")
        fl = 2.0 * P * D_ * D_ * B
        for name, mult in (("pnn_mat_fwd_kernel", 1), ("pnn_mat_dx_kernel", 2), ("pnn_mat_dk_kernel", 1)):
            us = next((u for n, u in per if n == name), None)
            if us:
                print(f"{name}: {mult * fl / 1e9:.2f} GFLOP in {us:.1f} us = {mult * fl / us / 1e6:.1f} TFLOP/s, "
                      f"{100 * mult * fl / us / 1e6 / PEAK_TFLOPS:.1f} % of the {PEAK_TFLOPS:.1f} TFLOP/s fp32 matrix peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnn_time.txt"))
    ap.add_argument("--batch", type=int, default=None, help="(internal) run one batch size in this process")
    ap.add_argument("--config", default=None, help="(internal) with --batch: one of " + ", ".join(CONFIGS))
    a = ap.parse_args()
    if a.batch is not None:
        run(a.batch, a.config, a.reps, a.inner)
        return
    text = [f"tools/pnn_time.py; median (min - max) of {a.reps} alternating rounds of {a.inner} calls"]      # (no GPU use here)
    for B in BATCHES:      # a child process per leg, each under its own time limit; nothing starts after a failure
        for config in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--config", config, "--reps", str(a.reps),
                   "--inner", str(a.inner)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"B = {B}, {config}: no result within {CHILD_LIMIT_S} s; stopping")
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"B = {B}, {config}: exit status {r.returncode}; stopping")
            text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
