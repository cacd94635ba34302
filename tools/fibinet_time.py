"""Cost of the FiBiNET head (csrc/fibinet.hip) at the AliCCP shape - F = 19 fields, D = 32, bilinear_type 'interaction',
reduction_ratio 3, dnn_hidden_units (128, 128): P = 171 pairs, a DNN input of 10,944 columns - at B = 4096 and B = 8192, against
the same head written as torch ops on the same GPU: deepctr's form, a Linear, a mul per pair and a 171-way cat for each of the two
blocks, a torch DNN, autograd - what a port of FiBiNET runs without these kernels.  That baseline is not the code under test.
Writes profiles/fibinet_time.txt, per batch size:
  - the library's forward (satrans_fibinet_fwd) and forward + backward (then satrans_fibinet_bwd) on preallocated buffers:
    device events around the calls, so kernels only, no host work between;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - FiBiNETHead forward + backward as a user calls it (autograd, the stack of the bilinear weights, allocation of the saved and
    work buffers included) and the torch form, by the host's clock around a device synchronise;
    all legs in ALTERNATING rounds, library then torch; median (min - max) over the rounds;
  - every launch of one library forward + backward in launch order with its own duration (torch.profiler's device records,
    median over the profiled calls); from them the share of the fp32 matrix peak that the DNN's first layer reaches (2 B n 128
    FLOP over its forward launch) and the share of the HBM peak that the bilinear forward's stores reach (8 B P D bytes over its
    launch);
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two logits, relative to max|logit|.
Each batch size runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/fibinet_time.py [--reps 10] [--inner 3] [--out profiles/fibinet_time.txt]"""
import argparse
import ctypes
import itertools
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F_, D_, KIND, RATIO, DNN = 19, 32, "interaction", 3, (128, 128)
BATCHES = (4096, 8192)
PEAK_TFLOPS = 155.0      # fp32 matrix peak of the MI355X
PEAK_HBM_TBS = 8.0       # HBM3E peak of the MI355X
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


def run(B, reps, inner):
    import torch
    import torch.nn.functional as Fn
    from satrans_amd import FiBiNETHead, layers, native as N
    lib = N.lib()
    P = F_ * (F_ - 1) // 2
    n_in = 2 * P * D_
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== B = {B}, F = {F_}, D = {D_}, '{KIND}', reduction_ratio {RATIO}, dnn {DNN}: P = {P}, DNN input {n_in} columns"]
    torch.manual_seed(B)
    head = FiBiNETHead(F_, D_, 0, KIND, RATIO, DNN, init_std=n_in ** -0.5).to(DEV)
    with torch.no_grad():
        for w in (head.SE.excitation[0].weight, head.SE.excitation[2].weight):
            w.abs_()      # open gates
    emb = torch.randn(B, F_, D_, device=DEV, requires_grad=True)
    up = torch.randn(B, 1, device=DEV)
    pairs = list(itertools.combinations(range(F_), 2))

    def clear():
        head.zero_grad(set_to_none=True)
        emb.grad = None

    def bilinear_torch(x):      # deepctr's 'interaction' form
        xs = torch.split(x, 1, dim=1)
        return torch.cat([torch.mul(lin(xs[i]), xs[j]) for (i, j), lin in zip(pairs, head.Bilinear.bilinear)], dim=1)

    def torch_f():
        A = head.SE.excitation(torch.mean(emb, dim=-1))
        V = torch.mul(emb, torch.unsqueeze(A, dim=2))
        h = torch.flatten(torch.cat((bilinear_torch(V), bilinear_torch(emb)), dim=1), start_dim=1)
        for lin in head.dnn.linears:
            h = torch.relu(lin(h))
        return head.dnn_linear(h) + head.out.bias

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    def mod_fb():
        clear()
        (head(emb) * up).sum().backward()

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        bil_w = torch.stack(head.Bilinear.weights())
        dnn = [l.weight.detach() for l in head.dnn.linears] + [l.bias.detach() for l in head.dnn.linears]
        tensors = (head.SE.excitation[0].weight.detach(), head.SE.excitation[2].weight.detach(), bil_w, dnn,
                   head.dnn_linear.weight.detach(), head.out.bias.detach())
        xd = emb.detach().contiguous()
        d = layers._fibinet_desc(xd, None, N.BILINEAR_TYPES[KIND], *tensors)
        saved = torch.empty(int(lib.satrans_fibinet_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        work = torch.empty(int(lib.satrans_fibinet_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
        logit, demb = torch.empty(B, 1, device=DEV), torch.empty_like(xd)
        grads = [torch.empty_like(t) for t in (tensors[0], tensors[1], bil_w, *dnn, tensors[4], tensors[5])]
        g = layers._fibinet_fill(N.FiBiNETGrads(), len(DNN), grads[0], grads[1], grads[2], grads[3:-2], grads[-2], grads[-1])
    stream = N.stream_handle(torch.device(DEV))

    def lib_f():
        N.check(lib.satrans_fibinet_fwd(ctypes.byref(d), logit.data_ptr(), saved.data_ptr(), stream), "satrans_fibinet_fwd")

    def lib_fb():
        lib_f()
        N.check(lib.satrans_fibinet_bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), None, saved.data_ptr(), work.data_ptr(),
                                        ctypes.byref(g), stream), "satrans_fibinet_bwd")

    with torch.no_grad():
        y_new, y_old = head(emb), torch_f()
    lines.append(f"largest |FiBiNETHead - torch form| / max|logit|: {float((y_new - y_old).abs().max() / y_old.abs().max()):.2e}")
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
    lines.append(f"FiBiNETHead module forward + backward (host clock): {fmt(s['w_new'])}")
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
        first_gemm = next((us for name, us in per if name == "mmoe_gemm_kernel"), None)
        bil = next((us for name, us in per if name == "fibinet_bil_fwd_kernel"), None)
        if first_gemm:
            fl = 2.0 * B * n_in * DNN[0]
            print(f"DNN first layer forward: {fl / 1e9:.1f} GFLOP in {first_gemm:.1f} us = {fl / first_gemm / 1e6:.1f} TFLOP/s, "
                  f"{100 * fl / first_gemm / 1e6 / PEAK_TFLOPS:.1f} % of the {PEAK_TFLOPS:.0f} TFLOP/s fp32 matrix peak")
        if bil:
            by = 4.0 * B * n_in
            print(f"bilinear forward stores: {by / 1e6:.1f} MB in {bil:.1f} us = {by / bil / 1e6:.2f} TB/s, "
                  f"{100 * by / bil / 1e6 / PEAK_HBM_TBS:.1f} % of the {PEAK_HBM_TBS:.0f} TB/s HBM peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fibinet_time.txt"))
    ap.add_argument("--batch", type=int, default=None, help="(internal) run one batch size in this process")
    a = ap.parse_args()
    if a.batch is not None:
        run(a.batch, a.reps, a.inner)
        return
    text = [f"tools/fibinet_time.py; median (min - max) of {a.reps} alternating rounds of {a.inner} calls"]
    for B in BATCHES:      # a child process per batch size, each under its own time limit; nothing starts after a failure
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
