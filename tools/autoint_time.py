"""Cost of AutoInt's interacting layers (csrc/autoint.hip) at the AliCCP shape - F = 19 fields, D = 32 - with H = 2 (AutoInt's
default) and H = 4 (SATrans's head count): one InteractingLayer, the 3-layer stack, and AutoIntHead with DNN (256, 128); at
B = 8192 (forward, and forward + backward) and B = 32768 (the forward alone); against the same thing written as torch ops on the
same GPU, fp32: deepctr's literal form (tests/autoint_reference.py: tensordot, split / stack over the heads, the einsum, softmax,
matmul, cat, relu), a torch DNN, autograd - what a port of AutoInt runs without the kernels.  That baseline is not the code
under test.  One INFORMATIVE leg: SelfAttention_Layer.eval() at the same shape, the nearest existing kernel path; its arithmetic
is different (W_Out, LayerNorm, scaling on), so its figures stand beside the layer's, not against them.
Writes profiles/autoint_time.txt, per leg, head count and batch size:
  - the library's forward and forward + backward on preallocated buffers: device events around the calls, so kernels only, no
    host work between;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - the module's forward + backward as a user calls it (autograd, allocation of the saved and work buffers included) and the
    torch form, by the host's clock around a device synchronise;
    all legs in ALTERNATING rounds, library then torch; median (min - max) over the rounds;
  - every launch of one library forward + backward in launch order with its own duration (torch.profiler's device records,
    median over the profiled calls); for the two layer kernels the bytes they move against the floor of reading x and writing y
    once, and their rate against the fp32 matrix peak;
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two results, relative to max|.|.
Each (leg, head count, batch size) runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/autoint_time.py [--reps 10] [--inner 3] [--out profiles/autoint_time.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F_, D_ = 19, 32
LEGS = ("layer", "stack", "head", "selfatt")
HEADS = (2, 4)
DNN = (256, 128)
BATCHES = ((8192, True), (32768, False))      # (B, with the backward)
PEAK_MATRIX_TFLOPS = 157.3        # fp32 on the matrix pipe
HBM_TBS = 8.0                     # the MI355X's HBM3E peak
CHILD_LIMIT_S = 240
DEV = "cuda:0"


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def fmt(t, unit="ms"):
    return f"median {t[0]:.4f} {unit} ({t[1]:.4f} - {t[2]:.4f})"


def disjoint(lo, hi):
    return "ranges disjoint" if lo[2] < hi[1] or hi[2] < lo[1] else "ranges OVERLAP"


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


def run(leg, H, B, with_bwd, reps, inner):
    import torch
    from satrans_amd import AutoIntHead, InteractingLayer, SelfAttention_Layer, layers, native as N
    from tests import autoint_reference as R
    lib = N.lib()
    n_layers = 1 if leg in ("layer", "selfatt") else 3
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== '{leg}', H = {H}, B = {B}{'' if with_bwd else ' (forward alone)'}: F = {F_}, D = {D_}, {n_layers} layer(s)" +
             (f", dnn {DNN}" if leg == "head" else "") +
             (" -- INFORMATIVE: SelfAttention_Layer.eval(), other arithmetic (W_Out, LayerNorm, scaling)" if leg == "selfatt" else "")]
    torch.manual_seed(B + H)
    emb = torch.randn(B, F_, D_, device=DEV, requires_grad=True)
    stream = N.stream_handle(torch.device(DEV))
    if leg == "head":
        mod = AutoIntHead(F_, D_, 0, 3, H, True, DNN, init_std=(F_ * D_) ** -0.5).to(DEV)
        int_layers = list(mod.int_layers)
    elif leg == "selfatt":
        mod = SelfAttention_Layer(D_, H).to(DEV).eval()
        int_layers = []
    else:
        int_layers = [InteractingLayer(D_, H).to(DEV) for _ in range(n_layers)]
        mod = torch.nn.Sequential(*int_layers)
    with torch.no_grad():      # weights of a visible size: N(0, 1 / D), as in the tests' draws
        for layer in int_layers:
            for w in layer.weights():
                w.normal_(0.0, D_ ** -0.5)
    up = torch.randn((B, 1) if leg == "head" else (B, F_, D_), device=DEV)

    def clear():
        mod.zero_grad(set_to_none=True)
        emb.grad = None

    def mod_f():
        return mod(emb)

    def torch_f():      # deepctr's literal form over the module's own parameters
        if leg == "head":
            return R.forward(emb, None, R.params_from_state(dict(mod.named_parameters()), torch.float32), H)[0]
        return R.stack_forward(emb, [dict(layer.named_parameters()) for layer in int_layers], H)[0]

    def mod_fb():
        clear()
        (mod_f() * up).sum().backward()

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    if leg == "selfatt":      # the module alone, forward and forward + backward
        mod_f()
        mem = peak_mb(mod_fb if with_bwd else mod_f)
        for fn in (mod_f, mod_fb):
            fn()
        got = {"f": [], "fb": [], "w": []}
        for _ in range(reps):
            got["f"].append(event_ms(mod_f, inner))
            if with_bwd:
                got["fb"].append(event_ms(mod_fb, inner))
            got["w"].append(wall_ms(mod_fb if with_bwd else mod_f, inner))
        lines.append(f"module forward (device events, host work between the launches included): {fmt(stats(got['f']))}")
        if with_bwd:
            lines.append(f"module forward + backward (device events, likewise):                     {fmt(stats(got['fb']))}")
        lines.append(f"module {'forward + backward' if with_bwd else 'forward'} (host clock): {fmt(stats(got['w']))}")
        lines.append(f"peak memory above the start: {mem:.1f} MB")
        print("\n".join(lines), flush=True)
        per = launches(mod_fb if with_bwd else mod_f, 5)
        if per:
            print(f"launches of one module call, in launch order (median us of 5 profiled calls; sum {sum(u for _, u in per):.1f} us):")
            for i, (name, us) in enumerate(per):
                print(f"  {i:2d}  {name:28s} {us:9.1f}")
        return

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        xd = emb.detach().contiguous()
        if leg == "head":
            tensors = [w.detach() for layer in int_layers for w in layer.weights()]
            ws = [l.weight.detach() for l in mod.dnn.linears] + [l.bias.detach() for l in mod.dnn.linears]
            lin_w, out_b = mod.dnn_linear.weight.detach(), mod.out.bias.detach()
            cfg = (H, layers._interacting_flags(True, False), 3, (False,) * 3)
            d = layers._autoint_desc(xd, None, cfg, tensors, ws, lin_w, out_b)
            saved = torch.empty(int(lib.satrans_autoint_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            work = torch.empty(int(lib.satrans_autoint_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            out, demb = torch.empty(B, 1, device=DEV), torch.empty_like(xd)
            g_int = torch.empty(3, 4, D_, D_, device=DEV)
            grads = [torch.empty_like(t) for t in ws] + [torch.empty_like(lin_w), torch.empty_like(out_b)]
            g = layers._autoint_fill(N.AutoIntGrads(), len(DNN), grads[:-2], grads[-2], grads[-1])
            for l in range(3):
                g.int_w[l] = g_int[l].data_ptr()

            def lib_f():
                N.check(lib.satrans_autoint_fwd(ctypes.byref(d), out.data_ptr(), None, saved.data_ptr(), stream), "satrans_autoint_fwd")

            def lib_b():
                N.check(lib.satrans_autoint_bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), None, saved.data_ptr(), work.data_ptr(),
                                                ctypes.byref(g), stream), "satrans_autoint_bwd")
        else:
            flags = layers._interacting_flags(True, False)
            xs = [xd] + [torch.empty_like(xd) for _ in range(n_layers)]
            gs = [torch.empty_like(xd) for _ in range(2)]
            descs = [layers._interacting_desc(xs[l], H, flags, [w.detach() for w in int_layers[l].weights()]) for l in range(n_layers)]
            n_saved = int(lib.satrans_interacting_saved_floats(ctypes.byref(descs[0])))
            saved = torch.empty(n_layers * n_saved, dtype=torch.float32, device=DEV)
            work = torch.empty(int(lib.satrans_interacting_scratch_floats(ctypes.byref(descs[0]))), dtype=torch.float32, device=DEV)
            g_int = torch.empty(n_layers, 4, D_, D_, device=DEV)

            def lib_f():
                for l in range(n_layers):
                    N.check(lib.satrans_interacting_fwd(ctypes.byref(descs[l]), xs[l + 1].data_ptr(), None,
                                                        saved.data_ptr() + 4 * l * n_saved, stream), "satrans_interacting_fwd")

            def lib_b():
                dy = up
                for l in range(n_layers - 1, -1, -1):
                    N.check(lib.satrans_interacting_bwd(ctypes.byref(descs[l]), xs[l + 1].data_ptr(), dy.data_ptr(), gs[l & 1].data_ptr(),
                                                        saved.data_ptr() + 4 * l * n_saved, work.data_ptr(), g_int[l].data_ptr(), stream),
                            "satrans_interacting_bwd")
                    dy = gs[l & 1]

    def lib_fb():
        lib_f()
        lib_b()

    with torch.no_grad():
        y_new, y_old = mod_f(), torch_f()
    lines.append(f"largest |module - torch form| / max|.|: {float((y_new - y_old).abs().max() / y_old.abs().max()):.2e}")
    legs = {"k_f": lib_f, "t_f": torch_f}
    if with_bwd:
        mem_new, mem_old = peak_mb(mod_fb), peak_mb(torch_fb)
        legs.update({"k_fb": lib_fb, "t_fb": torch_fb})
    else:
        mem_new, mem_old = peak_mb(mod_f), peak_mb(torch_f)
    wall = (mod_fb, torch_fb) if with_bwd else (mod_f, torch_f)
    for fn in (*legs.values(), *wall):      # warm-up
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in (*legs, "w_new", "w_old")}
    for _ in range(reps):      # alternating rounds: library, torch, library, torch, ..
        for k, fn in legs.items():
            got[k].append(event_ms(fn, inner))
        got["w_new"].append(wall_ms(wall[0], inner))
        got["w_old"].append(wall_ms(wall[1], inner))
    s = {k: stats(v) for k, v in got.items()}
    what = "forward + backward" if with_bwd else "forward"
    lines.append(f"library forward (device events):                    {fmt(s['k_f'])}")
    lines.append(f"torch form forward (device events):                 {fmt(s['t_f'])}    torch / library = "
                 f"{s['t_f'][0] / s['k_f'][0]:.2f}, {disjoint(s['k_f'], s['t_f'])}")
    if with_bwd:
        lines.append(f"library forward + backward (device events):         {fmt(s['k_fb'])}")
        lines.append(f"torch form forward + backward (device events):      {fmt(s['t_fb'])}    torch / library = "
                     f"{s['t_fb'][0] / s['k_fb'][0]:.2f}, {disjoint(s['k_fb'], s['t_fb'])}")
    lines.append(f"module {what} (host clock):{' ' * (33 - len(what))}{fmt(s['w_new'])}")
    lines.append(f"torch form {what} (host clock):{' ' * (29 - len(what))}{fmt(s['w_old'])}    torch / module = "
                 f"{s['w_old'][0] / s['w_new'][0]:.2f}, {disjoint(s['w_new'], s['w_old'])}")
    lines.append(f"peak memory above the start, {what}: module {mem_new:.1f} MB, torch form {mem_old:.1f} MB    "
                 f"torch / module = {mem_old / max(mem_new, 1e-9):.1f}")
    lines.append(f"(input [B, {F_}, {D_}] fp32: {B * F_ * D_ * 4 / 1e6:.1f} MB; saved {saved.numel() * 4 / 1e6:.1f} MB, workspace "
                 f"{work.numel() * 4 / 1e6:.1f} MB)")
    print("\n".join(lines), flush=True)
    per = launches(lib_fb if with_bwd else lib_f, 5)
    if per:
        total = sum(us for _, us in per)
        print(f"launches of one library {what}, in launch order (median us of 5 profiled calls; sum {total:.1f} us):")
        for i, (name, us) in enumerate(per):
            print(f"  {i:2d}  {name:28s} {us:9.1f}")
        xy = 2 * B * F_ * D_ * 4      # the floor: x read once, y written once
        st = 2 * B * H * F_ * 4
        part = work.numel() * 4 if leg != "head" else 0
        fl_f = 2.0 * B * F_ * D_ * 4 * D_ + 4.0 * B * F_ * F_ * D_      # the product, then scores and p v
        for name, moved, fl in (("int_fwd_kernel", xy + st + 4 * D_ * D_ * 4, fl_f),
                                ("int_bwd_kernel", 2 * xy + st + 4 * D_ * D_ * 4 + part, 2.5 * fl_f)):
            us = next((u for n, u in per if n == name), None)
            if us:
                floor_us = xy / (HBM_TBS * 1e6)
                print(f"{name}: moves {moved / 1e6:.1f} MB (x + y floor {xy / 1e6:.1f} MB = {floor_us:.1f} us at {HBM_TBS:.0f} TB/s) in "
                      f"{us:.1f} us = {us / floor_us:.1f} x the floor, {moved / us / 1e6:.2f} TB/s; {fl / 1e9:.2f} GFLOP = "
                      f"{fl / us / 1e6:.1f} TFLOP/s, {100 * fl / us / 1e6 / PEAK_MATRIX_TFLOPS:.1f} % of the {PEAK_MATRIX_TFLOPS:.1f} "
                      f"TFLOP/s fp32 matrix peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoint_time.txt"))
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process: one of " + ", ".join(LEGS))
    ap.add_argument("--heads", type=int, default=None, help="(internal) with --leg: the head count")
    ap.add_argument("--batch", type=int, default=None, help="(internal) with --leg: the batch size")
    ap.add_argument("--forward-only", action="store_true", help="(internal) with --leg: the forward alone")
    a = ap.parse_args()
    if a.leg is not None:
        run(a.leg, a.heads, a.batch, not a.forward_only, a.reps, a.inner)
        return
    text = [f"tools/autoint_time.py; median (min - max) of {a.reps} alternating rounds of {a.inner} calls"]      # (no GPU use here)
    for leg in LEGS:      # a child process per leg, head count and batch size, each under its own time limit; nothing starts after a failure
        for H in HEADS:
            for B, with_bwd in BATCHES:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--heads", str(H), "--batch", str(B), "--reps",
                       str(a.reps), "--inner", str(a.inner)] + ([] if with_bwd else ["--forward-only"])
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"{leg}, H = {H}, B = {B}: no result within {CHILD_LIMIT_S} s; stopping")
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"{leg}, H = {H}, B = {B}: exit status {r.returncode}; stopping")
                text.append(r.stdout.rstrip())
                print(f"[autoint_time] {leg}, H = {H}, B = {B}: done", file=sys.stderr, flush=True)
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
