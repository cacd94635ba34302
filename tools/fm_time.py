"""Cost of FM, BiInteractionPooling and the AFM, DeepFM and NFM heads (csrc/fm.hip) at the AliCCP shape - F = 19 fields, D = 32:
P = 171 pairs; attention factor A = 8; DNN (256, 128) for DeepFM and (128, 128) for NFM - at B = 8192 (forward, and forward +
backward) and B = 32768 (the forward alone); against the same layer or head written as torch ops on the same GPU, fp32:
deepctr's literal form (tests/fm_reference.py: for AFM the two gathered [B, P, D] tensors, tensordot, softmax over dim 1), a torch
DNN, autograd - what a port of these models runs without the kernels.  That baseline is not the code under test.
Writes profiles/fm_time.txt, per leg and batch size:
  - the library's forward and forward + backward on preallocated buffers: device events around the calls, so kernels only, no
    host work between;
  - the torch form's forward (autograd on, as in training) and forward + backward, likewise between device events;
  - the module's forward + backward as a user calls it (autograd, allocation of the saved and work buffers included) and the
    torch form, by the host's clock around a device synchronise;
    all legs in ALTERNATING rounds, library then torch; median (min - max) over the rounds;
  - every launch of one library forward + backward in launch order with its own duration (torch.profiler's device records,
    median over the profiled calls), and for the two AFM kernels their rate against the input read and the fp32 vector peak;
  - the peak of torch's allocator over one forward + backward above what was allocated before, both sides;
  - the largest difference between the two results, relative to max|.|.
Each (leg, batch size) runs in a child process of its own under a time limit; nothing starts after a failure.
Usage: python tools/fm_time.py [--reps 10] [--inner 3] [--out profiles/fm_time.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F_, D_, A_ = 19, 32, 8
LEGS = {"afm": (), "deepfm": (256, 128), "nfm": (128, 128), "fm": (), "bipool": ()}      # leg -> dnn_hidden_units
BATCHES = ((8192, True), (32768, False))      # (B, with the backward)
PEAK_VALU_TFLOPS = 157.3 / 2      # fp32 FMA on the vector pipe, unpacked
HBM_TBS = 8.0                     # the MI355X's HBM3E peak
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


def run(leg, B, with_bwd, reps, inner):
    import torch
    from satrans_amd import FM, AFMHead, BiInteractionPooling, DeepFMHead, NFMHead, layers, native as N
    from tests import fm_reference as R
    lib = N.lib()
    dnn = LEGS[leg]
    P = F_ * (F_ - 1) // 2
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"== '{leg}', B = {B}{'' if with_bwd else ' (forward alone)'}: F = {F_}, D = {D_}, P = {P}" +
             (f", A = {A_}" if leg == "afm" else "") + (f", dnn {dnn}" if dnn else "")]
    torch.manual_seed(B)
    n_in = (D_ if leg == "nfm" else F_ * D_)
    mod = {"afm": lambda: AFMHead(D_, A_), "deepfm": lambda: DeepFMHead(F_, D_, 0, True, dnn, init_std=n_in ** -0.5),
           "nfm": lambda: NFMHead(D_, 0, dnn, init_std=n_in ** -0.5), "fm": FM, "bipool": BiInteractionPooling}[leg]().to(DEV)
    head = leg in ("afm", "deepfm", "nfm")
    emb = torch.randn(B, F_, D_, device=DEV, requires_grad=True)
    lin = torch.randn(B, 1, device=DEV)
    up = torch.randn((B, 1, D_) if leg == "bipool" else (B, 1), device=DEV)
    stream = N.stream_handle(torch.device(DEV))

    def clear():
        mod.zero_grad(set_to_none=True)
        emb.grad = None

    def mod_f():
        return mod(emb, lin) if leg == "afm" else mod(emb, None, lin) if head else mod(emb)

    def torch_f():      # deepctr's literal form over the module's own parameters
        if leg == "fm":
            return R.fm(emb)
        if leg == "bipool":
            return R.bipool(emb)
        Pm = R.params_from_state(dict(mod.named_parameters()), torch.float32)
        return R.forward(leg, emb, None, lin, Pm)[0]

    def torch_fb():
        clear()
        (torch_f() * up).sum().backward()

    def mod_fb():
        clear()
        (mod_f() * up).sum().backward()

    # the library calls alone, on preallocated buffers
    with torch.no_grad():
        xd = emb.detach().contiguous()
        demb = torch.empty_like(xd)
        if leg == "afm":
            params = [p.detach() for p in (mod.fm.attention_W, mod.fm.attention_b, mod.fm.projection_h, mod.fm.projection_p)]
            d = layers._afm_desc(xd, params, lin, mod.out.bias.detach())
            saved = torch.empty(int(lib.satrans_afm_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            work = torch.empty(int(lib.satrans_afm_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            out = torch.empty(B, 1, device=DEV)
            grads =[torch.empty_like(p) for p in params] + [torch.empty(1, device=DEV)]
            g = layers._afm_fill(N.AFMGrads(), grads[:4], grads[4])

            def lib_f():
                N.check(lib.satrans_afm_fwd(ctypes.byref(d), out.data_ptr(), saved.data_ptr(), stream), "satrans_afm_fwd")

            def lib_b():
                N.check(lib.satrans_afm_bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                            ctypes.byref(g), stream), "satrans_afm_bwd")
        elif head:
            ws = [l.weight.detach() for l in mod.dnn.linears] + [l.bias.detach() for l in mod.dnn.linears]
            lin_w, out_b = mod.dnn_linear.weight.detach(), mod.out.bias.detach()
            cfg = (N.FMHEAD_NFM, 0) if leg == "nfm" else (N.FMHEAD_DEEPFM, 1)
            d = layers._fmhead_desc(xd, None, lin, cfg, ws, lin_w, out_b)
            saved = torch.empty(int(lib.satrans_fmhead_saved_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            work = torch.empty(int(lib.satrans_fmhead_workspace_floats(ctypes.byref(d))), dtype=torch.float32, device=DEV)
            out = torch.empty(B, 1, device=DEV)
            grads = [torch.empty_like(t) for t in ws] + [torch.empty_like(lin_w), torch.empty_like(out_b)]
            g = layers._fmhead_fill(N.FMHeadGrads(), len(dnn), grads[:-2], grads[-2], grads[-1])

            def lib_f():
                N.check(lib.satrans_fmhead_fwd(ctypes.byref(d), out.data_ptr(), saved.data_ptr(), stream), "satrans_fmhead_fwd")

            def lib_b():
                N.check(lib.satrans_fmhead_bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), None, saved.data_ptr(), work.data_ptr(),
                                               ctypes.byref(g), stream), "satrans_fmhead_bwd")
        else:
            d = layers._fm_desc(xd)
            saved = work = torch.empty(0, device=DEV)
            out = torch.empty_like(up)
            fwd, bwd = (lib.satrans_fm_fwd, lib.satrans_fm_bwd) if leg == "fm" else (lib.satrans_bipool_fwd, lib.satrans_bipool_bwd)

            def lib_f():
                N.check(fwd(ctypes.byref(d), out.data_ptr(), stream), f"satrans_{leg}_fwd")

            def lib_b():
                N.check(bwd(ctypes.byref(d), up.data_ptr(), demb.data_ptr(), stream), f"satrans_{leg}_bwd")

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
    lines.append(f"(input [B, {F_}, {D_}] fp32: {B * F_ * D_ * 4 / 1e6:.1f} MB; [B, P, D]: {B * P * D_ * 4 / 1e6:.1f} MB; saved "
                 f"{saved.numel() * 4 / 1e6:.1f} MB, workspace {work.numel() * 4 / 1e6:.1f} MB)")
    print("\n".join(lines), flush=True)
    per = launches(lib_fb if with_bwd else lib_f, 5)
    if per:
        total = sum(us for _, us in per)
        print(f"launches of one library {what}, in launch order (median us of 5 profiled calls; sum {total:.1f} us):")
        for i, (name, us) in enumerate(per):
            print(f"  {i:2d}  {name:28s} {us:9.1f}")
        read_us = B * F_ * D_ * 4 / (HBM_TBS * 1e6)
        fl = 2.0 * B * P * D_ * A_
        for name, mult in (("afm_fwd_kernel", 1), ("afm_bwd_kernel", 3)):
            us = next((u for n, u in per if n == name), None)
            if us:
                print(f"{name}: {mult * fl / 1e9:.2f} GFLOP in {us:.1f} us = {mult * fl / us / 1e6:.1f} TFLOP/s, "
                      f"{100 * mult * fl / us / 1e6 / PEAK_VALU_TFLOPS:.1f} % of the {PEAK_VALU_TFLOPS:.1f} TFLOP/s fp32 vector peak; "
                      f"{us / read_us:.1f} x the {read_us:.1f} us of reading the input once at {HBM_TBS:.0f} TB/s")
        for name in ("fm_rows_fwd_kernel", "fm_rows_bwd_kernel"):
            us = next((u for n, u in per if n == name), None)
            if us:
                print(f"{name}: {us:.1f} us = {us / read_us:.1f} x the {read_us:.1f} us of reading the input once at {HBM_TBS:.0f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_time.txt"))
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process: one of " + ", ".join(LEGS))
    ap.add_argument("--batch", type=int, default=None, help="(internal) with --leg: the batch size")
    ap.add_argument("--forward-only", action="store_true", help="(internal) with --leg: the forward alone")
    a = ap.parse_args()
    if a.leg is not None:
        run(a.leg, a.batch, not a.forward_only, a.reps, a.inner)
        return
    text = [f"tools/fm_time.py; median (min - max) of {a.reps} alternating rounds of {a.inner} calls"]      # (no GPU use here)
    for leg in LEGS:      # a child process per leg and batch size, each under its own time limit; nothing starts after a failure
        for B, with_bwd in BATCHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(B), "--reps", str(a.reps),
                   "--inner", str(a.inner)] + ([] if with_bwd else ["--forward-only"])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{leg}, B = {B}: no result within {CHILD_LIMIT_S} s; stopping")
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{leg}, B = {B}: exit status {r.returncode}; stopping")
            text.append(r.stdout.rstrip())
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
