"""Cost of the partitioned normalisation (csrc/pnorm.hip) at B = 8192, S = 4: C = 608 (AliCCP's head width, 19 fields x 32) and
C = 64, against the reference's form on the same GPU - the loop of models/star.py:147-154 as torch ops: boolean-mask select,
F.batch_norm on the selected rows, masked write-back, once per scenario.
Writes profiles/mdr_bn_time.txt:
  - PartitionedNorm forward and forward + backward, training mode, as a user calls it (bucketing, the one device-to-host read
    of the segment bounds, the stacking of the per-scenario parameters and autograd included);
  - the launches of satrans_pnorm_fwd / satrans_pnorm_bwd alone, the bytes of their roofline (x read + y written; x, dy read +
    y, dx written) and the fraction of the HBM peak that is;
  - the torch loop, forward and forward + backward.
Device events around `--inner` calls, warmed, median of `--reps` repetitions.
Usage: python tools/mdr_bn_time.py [--reps 30] [--inner 10] [--out profiles/mdr_bn_time.txt]"""
import argparse
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from satrans_amd import PartitionedNorm, native as N  # noqa: E402
from satrans_amd.layers import _pnorm_desc  # noqa: E402

B, S = 8192, 4
HBM_PEAK_GBS = 8000.0                  # MI355X HBM3E peak; a float4 copy reaches 6,290 GB/s (MI355X_MICROARCH.md)
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def events_us(fn, reps, inner):
    for _ in range(3 * inner):
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


def torch_loop(bns, x, ids, sw, sb):
    out = torch.zeros_like(x)
    for d, bn in enumerate(bns):
        rows = ids == d
        out[rows] = F.batch_norm(x[rows], bn.running_mean, bn.running_var, bn.weight * sw, bn.bias + sb, True, 0.1, 1e-5)
    return out


def fmt(t):
    return f"median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def run(Cn, reps, inner, lines):
    g = torch.Generator().manual_seed(Cn)
    x = (torch.randn(B, Cn, generator=g) * 1.5 + 0.5).to(DEV).requires_grad_(True)
    w = torch.randn(B, Cn, generator=g).to(DEV)
    ids = torch.randint(0, S, (B,), generator=g).to(DEV)
    sw, sb = torch.ones(Cn, device=DEV, requires_grad=True), torch.zeros(Cn, device=DEV, requires_grad=True)
    mod = PartitionedNorm(Cn, S).to(DEV).train()
    twin = PartitionedNorm(Cn, S).to(DEV).train()
    lines.append(f"== B = {B}, C = {Cn}, S = {S} (rows per scenario: {torch.bincount(ids, minlength=S).tolist()})")

    def fwd():
        with torch.no_grad():
            mod(x, ids, sw, sb)

    def fwd_bwd():
        (mod(x, ids, sw, sb) * w).sum().backward()

    def loop_fwd():
        with torch.no_grad():
            torch_loop(twin.bns, x, ids, sw, sb)

    def loop_fwd_bwd():
        (torch_loop(twin.bns, x, ids, sw, sb) * w).sum().backward()

    y_new, y_old = mod(x, ids, sw, sb), torch_loop(twin.bns, x, ids, sw, sb)
    lines.append(f"largest |PartitionedNorm - torch loop| on these rows: {float((y_new - y_old).abs().max()):.2e}")
    t_f, t_fb = events_us(fwd, reps, inner), events_us(fwd_bwd, reps, inner)
    l_f, l_fb = events_us(loop_fwd, reps, inner), events_us(loop_fwd_bwd, reps, inner)
    lines.append(f"PartitionedNorm forward (module call):            {fmt(t_f)}")
    lines.append(f"torch loop forward:                               {fmt(l_f)}    loop / one pass = {l_f[0] / t_f[0]:.2f}")
    lines.append(f"PartitionedNorm forward + backward (module call): {fmt(t_fb)}")
    lines.append(f"torch loop forward + backward:                    {fmt(l_fb)}    loop / one pass = {l_fb[0] / t_fb[0]:.2f}")

    # the launches alone
    lib = N.lib()
    i32 = dict(dtype=torch.int32, device=DEV)
    sid, order, seg, status = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(S + 1, **i32), torch.zeros(1, **i32)
    bucket = torch.empty(int(lib.satrans_bucket_workspace_bytes(B, S)), dtype=torch.uint8, device=DEV)
    st = N.stream_handle(torch.device(DEV))
    N.check(lib.satrans_bucket_scenarios(ids.to(torch.int32).data_ptr(), N.ID_I32, 1, 0, B, S, sid.data_ptr(), order.data_ptr(),
                                         seg.data_ptr(), status.data_ptr(), bucket.data_ptr(), bucket.numel(), st), "bucket")
    xd = x.detach()
    P = [torch.ones(S, Cn, device=DEV), torch.zeros(S, Cn, device=DEV), sw.detach(), sb.detach()]
    rm, rv = torch.zeros(S, Cn, device=DEV), torch.ones(S, Cn, device=DEV)
    d = _pnorm_desc(xd, P[0], P[1], P[2], P[3], order, seg, rm, rv, 0.1, 1e-5, True)
    saved = torch.empty(int(lib.satrans_pnorm_saved_floats(C.byref(d))), device=DEV)
    work = torch.empty(int(lib.satrans_pnorm_workspace_floats(C.byref(d))), device=DEV)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    gr = [torch.empty(S, Cn, device=DEV), torch.empty(S, Cn, device=DEV), torch.empty(Cn, device=DEV), torch.empty(Cn, device=DEV)]

    def k_fwd():
        N.check(lib.satrans_pnorm_fwd(C.byref(d), y.data_ptr(), saved.data_ptr(), work.data_ptr(), st), "fwd")

    def k_bwd():
        N.check(lib.satrans_pnorm_bwd(C.byref(d), w.data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(), gr[0].data_ptr(),
                                      gr[1].data_ptr(), gr[2].data_ptr(), gr[3].data_ptr(), st), "bwd")

    def k_both():
        k_fwd()
        k_bwd()

    k_f, k_fb = events_us(k_fwd, reps, inner), events_us(k_both, reps, inner)
    rows = B * Cn * 4
    for name, t, nbytes, what in (("satrans_pnorm_fwd (3 launches)", k_f, 2 * rows, "x read + y written"),
                                  ("satrans_pnorm_fwd + _bwd (6 launches)", k_fb, 4 * rows, "x, dy read + y, dx written")):
        gbs = nbytes / t[0] / 1e3
        lines.append(f"{name}: {fmt(t)}; roofline bytes {nbytes / 1e6:.1f} MB ({what}) = {gbs:.0f} GB/s = "
                     f"{gbs / HBM_PEAK_GBS:.3f} of the {HBM_PEAK_GBS:.0f} GB/s HBM peak; the roof itself is "
                     f"{nbytes / HBM_PEAK_GBS / 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mdr_bn_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mdr_bn_time.py measures on the GPU; there is none here")
    lines = [f"tools/mdr_bn_time.py on {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}; "
             f"device events around {a.inner} calls, median of {a.reps} repetitions, training mode"]
    for Cn in (608, 64):
        run(Cn, a.reps, a.inner, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
