"""Cost of one training step of FeatureEmbedding + LinearModel with the AliCCP columns of examples/aliccp_main.py (19 SparseFeat,
about 6.6 M rows in all, embedding_dim 32) at B = 8192 under the linear loss sum(W * emb) + sum(c * logit) - forward, backward
and the optimizer step of the tables, no head - on four routes over the same initial parameters and the same batches:

  (a) un-adopted modules (dense table gradients) stepped by torch.optim.Adam over their parameters
  (b) optim.TableAdam, lazy, flush_every = 32, the 1-wide linear tables by the dense satrans_adam_flat sweep
  (c) optim.TableAdam, streaming (lazy = False): every row every step
  (d) as (b) with the 1-wide linear tables lazy too (linear_lazy = True)

l2 = 0 on every route (the explicit regulariser term of route (a) would only add traffic to it).  Device events around
`--steps` steps (64: two flushes of the lazy routes lie inside), `--rounds` alternating rounds, median (min - max) per step.  A
route is called faster than another only where the two ranges are disjoint.  The measuring runs in a child process under a time
limit.  Writes profiles/table_adam_time.txt.
Usage: python tools/table_adam_time.py [--rounds 10] [--steps 64] [--out profiles/table_adam_time.txt] [--note TEXT]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, B = 32, 8192
CHILD_LIMIT_S = 840
DEV = "cuda:0"
N_BATCHES = 8


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternating_us(routes, rounds, steps):
    """[step functions] -> [(median, min, max)] in microseconds per step, the routes timed in turn."""
    import torch
    for fn in routes:
        for i in range(steps):
            fn(i)
    torch.cuda.synchronize()
    out = [[] for _ in routes]
    for _ in range(rounds):
        for fn, acc in zip(routes, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                fn(i)
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b) * 1e3 / steps)
    return [(median(v), min(v), max(v)) for v in out]


def fmt(t):
    return f"{t[0]:.1f} us ({t[1]:.1f} - {t[2]:.1f})"


def verdict(name_x, x, name_y, y):
    if x[2] < y[1]:
        return f"{name_x} is faster than {name_y}, {y[0] / x[0]:.2f}x by the medians (ranges disjoint)"
    if y[2] < x[1]:
        return f"{name_y} is faster than {name_x}, {x[0] / y[0]:.2f}x by the medians (ranges disjoint)"
    return f"{name_x} and {name_y}: the ranges overlap, neither is called faster"


def run(rounds, steps):
    import torch
    from examples.aliccp_main import DATA_MAX, SPARSE
    from satrans_amd import FeatureEmbedding, LinearModel, SparseFeat, TableAdam, build_input_features, native as N
    cols = [SparseFeat(f, vocabulary_size=int(DATA_MAX[f]) + 2, embedding_dim=D) for f in SPARSE]
    fi = build_input_features(cols)
    nf = len(cols)
    g = torch.Generator().manual_seed(2)
    batches = [(torch.stack([torch.randint(0, c.vocabulary_size, (B,), generator=g) for c in cols], 1).float().to(DEV),
                (torch.rand(B, nf, D, generator=g) + 0.5).to(DEV), (torch.rand(B, generator=g) + 0.5).to(DEV))
               for _ in range(N_BATCHES)]

    def modules():
        torch.manual_seed(1)
        return FeatureEmbedding(cols, fi, init_std=0.1, device=DEV), LinearModel(cols, fi, init_std=0.1, device=DEV)

    def route(opt_of):
        fe, lin = modules()
        opt = opt_of(fe, lin)

        def step(i):
            X, W, c = batches[i % N_BATCHES]
            opt.zero_grad(set_to_none=True)
            ((fe(X)[0] * W).sum() + (lin(X).squeeze(1) * c).sum()).backward()
            opt.step()
        return step

    kw = dict(lr=1e-3, l2_reg_embedding=0.0, l2_reg_linear=0.0, flush_every=32)
    names = ["(a) dense gradients + torch.optim.Adam", "(b) TableAdam lazy, linear tables dense", "(c) TableAdam streaming",
             "(d) TableAdam lazy, linear tables lazy"]
    routes = [route(lambda fe, lin: torch.optim.Adam(list(fe.parameters()) + list(lin.parameters()), lr=1e-3)),
              route(lambda fe, lin: TableAdam([fe, lin], lazy=True, linear_lazy=False, **kw)),
              route(lambda fe, lin: TableAdam([fe, lin], lazy=False, linear_lazy=False, **kw)),
              route(lambda fe, lin: TableAdam([fe, lin], lazy=True, linear_lazy=True, **kw))]
    rows = sum(int(DATA_MAX[f]) + 2 for f in SPARSE)
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"{nf} fields, {rows} rows in all, D = {D}, B = {B}, {N_BATCHES} batches in turn; l2 = 0; forward + backward + table step, "
             f"per step over {steps} steps"]
    t = alternating_us(routes, rounds, steps)
    for name, r in zip(names, t):
        lines.append(f"{name}: {fmt(r)}")
    lines.append(verdict("(b)", t[1], "(a)", t[0]))
    lines.append(verdict("(b)", t[1], "(c)", t[2]))
    lines.append(verdict("(d) linear lazy", t[3], "(b) linear dense", t[1]))
    lines.append(f"derived floor of route (a)'s sweep: eight passes over the {rows * D * 4 / 1e6:.0f} MB arena = "
                 f"{8 * rows * D * 4 / 1e9:.1f} GB, {8 * rows * D * 4 / 8e12 * 1e6:.0f} us at 8 TB/s")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_adam_time.txt"))
    ap.add_argument("--note", default=None, help="a line recorded with the measurements")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.child:
        run(a.rounds, a.steps)
        return
    text = [f"tools/table_adam_time.py; device events around {a.steps} steps, median (min - max) per step of {a.rounds} alternating rounds"]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--steps", str(a.steps)]
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
