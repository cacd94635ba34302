"""Cost of LinearModel (csrc/linear.hip) and FeatureEmbedding (the gather / sort / dense-gradient ABI behind one autograd.Function)
with the AliCCP columns of examples/aliccp_main.py (19 SparseFeat, about 6.6 M rows in all, embedding_dim 32), as a user calls
them, against the literal torch form on the same GPU and the same parameters (one F.embedding per field, cat, sum; autograd for
the backward - torch's own dense embedding gradient):

  LinearModel       forward (no_grad)         and forward + backward (sum(c * logit).backward())
  FeatureEmbedding  forward (no_grad)         and forward + backward (sum(C * emb).backward())

at B = 8192, and forward only at B = 32768.  Every library forward includes its one status read (a host synchronisation); the
torch form has none.  Also timed alone: zero-filling a [rows, D] fp32 buffer - what the dense gradient of the reference's
sparse=False semantics costs before a kernel of the backward has run - and its share of FeatureEmbedding's forward + backward;
and FeatureEmbedding's forward + backward with the other kernel of the dense gradient (dense_gradient = "grad_dense").

Device events around `--inner` calls on inputs made once, warmed; `--rounds` alternating rounds of the library form against the
torch form; median (min - max).  A leg is called faster only where the two ranges are disjoint.  The measuring runs in a child
process under a time limit.  Writes profiles/input_time.txt.
Usage: python tools/input_time.py [--rounds 10] [--inner 5] [--out profiles/input_time.txt] [--note TEXT]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 32
CHILD_LIMIT_S = 840
DEV = "cuda:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternating_us(pair, rounds, inner):
    """(library, torch) -> ((median, min, max), (median, min, max)) in microseconds per call, the two timed in turn."""
    import torch
    for fn in pair:
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(rounds):
        for fn, acc in zip(pair, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b) * 1e3 / inner)
    return tuple((median(v), min(v), max(v)) for v in out)


def fmt(t):
    return f"{t[0]:.1f} us ({t[1]:.1f} - {t[2]:.1f})"


def verdict(lib, ref):
    if lib[2] < ref[1]:
        return f"the library form is faster, {ref[0] / lib[0]:.2f}x by the medians (ranges disjoint)"
    if ref[2] < lib[1]:
        return f"the torch form is faster, {lib[0] / ref[0]:.2f}x by the medians (ranges disjoint)"
    return "the ranges overlap: neither is called faster"


def run(rounds, inner):
    import torch
    import torch.nn.functional as F
    from examples.aliccp_main import DATA_MAX, SPARSE
    from satrans_amd import FeatureEmbedding, LinearModel, SparseFeat, build_input_features, native as N
    cols = [SparseFeat(f, vocabulary_size=int(DATA_MAX[f]) + 2, embedding_dim=D) for f in SPARSE]
    fi = build_input_features(cols)
    torch.manual_seed(1)
    lin = LinearModel(cols, fi, init_std=0.1, device=DEV)
    emb = FeatureEmbedding(cols, fi, init_std=0.1, device=DEV)
    rows, nf = emb.arena.shape[0], len(cols)
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"{nf} fields, {rows} rows in all, D = {D}: the dense table gradient is {rows * D * 4 / 1e6:.0f} MB "
             f"(FeatureEmbedding), {rows * 4 / 1e6:.0f} MB (LinearModel)"]
    g = torch.Generator().manual_seed(2)

    def batch(B):
        X = torch.stack([torch.randint(0, c.vocabulary_size, (B,), generator=g) for c in cols], 1).float().to(DEV)
        return X, torch.randn(B, generator=g).to(DEV), torch.randn(B, nf, D, generator=g).to(DEV)

    def ids_of(X):
        return [X[:, fi[c.name][0]:fi[c.name][1]].long() for c in cols]

    def torch_linear(X):
        return torch.sum(torch.cat([F.embedding(i, lin.embedding_dict[c.embedding_name].weight) for c, i in zip(cols, ids_of(X))], -1), -1)

    def torch_emb(X):
        return torch.cat([F.embedding(i, emb.embedding_dict[c.embedding_name].weight) for c, i in zip(cols, ids_of(X))], 1)

    def fwd(fn, X):
        def call():
            with torch.no_grad():
                fn(X)
        return call

    def fwd_bwd(mod, fn, X, w):
        def call():
            mod.zero_grad(set_to_none=True)
            (fn(X) * w).sum().backward()
        return call

    for B, legs in ((8192, ("forward", "forward + backward")), (32768, ("forward",))):
        X, c, Cw = batch(B)
        with torch.no_grad():
            d_lin = float((lin(X) - torch_linear(X)).abs().max())
            d_emb = float((emb(X)[0] - torch_emb(X)).abs().max())
        lines.append(f"== B = {B}: largest |library - torch form|: linear_logit {d_lin:.2e}, emb {d_emb:.2e}")
        for name, mod, lib_fn, ref_fn, w in (("LinearModel", lin, lambda x: lin(x), torch_linear, c.reshape(-1, 1)),
                                             ("FeatureEmbedding", emb, lambda x: emb(x)[0], torch_emb, Cw)):
            for leg in legs:
                pair = (fwd(lib_fn, X), fwd(ref_fn, X)) if leg == "forward" else \
                    (fwd_bwd(mod, lib_fn, X, w), fwd_bwd(mod, ref_fn, X, w))
                t_lib, t_ref = alternating_us(pair, rounds, inner)
                lines.append(f"{name} {leg}: library {fmt(t_lib)}; torch form {fmt(t_ref)}; {verdict(t_lib, t_ref)}")
                if name == "FeatureEmbedding" and leg != "forward":
                    emb.dense_gradient = "grad_dense"
                    t_walk, _ = alternating_us(pair, rounds, inner)
                    emb.dense_gradient = "segment_sums"
                    lines.append(f"  the same with dense_gradient = 'grad_dense' (one lane group per run): library {fmt(t_walk)}")
                    buf = torch.empty(rows, D, dtype=torch.float32, device=DEV)
                    t_zero, _ = alternating_us((lambda: buf.zero_(), lambda: None), rounds, inner)
                    lines.append(f"  zero-filling the dense [rows, D] gradient alone: {fmt(t_zero)} = {100 * t_zero[0] / t_lib[0]:.0f} % of the "
                                 f"library's forward + backward (the reference's dense semantics, not the kernels)")
                    del buf
    lines.append(f"designed-to floor of the linear forward at B = 8192: B R = {8192 * nf} scattered 4-byte reads, each a 64-byte "
                 f"request = {8192 * nf * 64 / 1e6:.1f} MB, a few microseconds of HBM time: the launch and the status read bound it")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_time.txt"))
    ap.add_argument("--note", default=None, help="a line recorded with the measurements")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.child:
        run(a.rounds, a.inner)
        return
    text = [f"tools/input_time.py; device events around {a.inner} calls, median (min - max) of {a.rounds} alternating rounds"]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--inner", str(a.inner)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"no result within {CHILD_LIMIT_S} s; stopping")
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"exit status {r.returncode}; stopping")
    text.append(r.stdout.rstrip())
    if a.note:
        text.append(a.note)
    out = "\n".join(text) + "\n"
    print(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
