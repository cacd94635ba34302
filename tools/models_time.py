"""Cost of one training step of WDL and MMOE with the AliCCP columns of examples/aliccp_main.py (19 SparseFeat, about 6.6 M rows in
all, embedding_dim 32) at B = 8192, on two routes over the same modules, the same initial parameters and the same batches:

  (a) the hand-written loop: the model's forward, torch's sigmoid and F.binary_cross_entropy(reduction='sum'), their backward,
      TableAdam (no regulariser value) + torch.optim.Adam, and a per-step `.item()` of the loss as the reference's fit has
  (b) HeadModel.train_step: PointLoss (one launch for prediction, loss and gradient), TableAdam(track_regularizer=True) +
      torch.optim.Adam, the step total added on the device, no host read by the harness

No ratio is promised: the claim under test is fewer launches and no per-step host wait in (b), against the satrans_sum_f64
launches that tracking the regulariser's value adds.  Device events around `--steps` steps (64: two flushes of the lazy tables lie
inside), `--rounds` alternating rounds, median (min - max) per step; a route is called faster only where the two ranges are
disjoint.  The measuring runs in a child process under a time limit.  Writes profiles/models_time.txt.
Usage: python tools/models_time.py [--rounds 10] [--steps 64] [--out profiles/models_time.txt] [--note TEXT]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from table_adam_time import alternating_us, fmt, verdict  # noqa: E402

D, B = 32, 8192
CHILD_LIMIT_S = 840
DEV = "cuda:0"
N_BATCHES = 8
SCENARIOS = 3


def run(rounds, steps):
    import torch
    import torch.nn.functional as F
    from examples.aliccp_main import DATA_MAX, SPARSE
    from satrans_amd import MMOE, WDL, SparseFeat, TableAdam, native as N
    domain = '301'                                       # the scenario column: ids 1..3
    vocab = {f: int(DATA_MAX[f]) + 2 for f in SPARSE}
    cols = [SparseFeat(f, vocabulary_size=vocab[f], embedding_dim=D) for f in SPARSE]
    g = torch.Generator().manual_seed(2)
    draw = lambda c: torch.randint(1, 1 + SCENARIOS, (B,), generator=g) if c.name == domain else \
        torch.randint(0, c.vocabulary_size, (B,), generator=g)      # noqa: E731
    batches = [(torch.stack([draw(c) for c in cols], 1).float().to(DEV),
                (torch.rand(B, generator=g) < 0.04).float().to(DEV)) for _ in range(N_BATCHES)]

    def model_of(kind):
        if kind == "WDL":
            return WDL(cols, cols, seed=1, device=DEV, flag="", init_std=0.01)
        m = MMOE(cols, seed=1, device=DEV, flag="", init_std=0.01, task_types=["binary"] * SCENARIOS,
                 task_names=["ctr%d" % i for i in range(SCENARIOS)], domain_column=domain)
        m.domain_id_offset = 1
        return m

    def hand_written(kind):
        m = model_of(kind)
        m.train()
        tables = [m.embedding] + ([m.linear_model] if m._linear_in_forward else [])
        topt = TableAdam(tables, lr=1e-3, l2_reg_embedding=1e-5, l2_reg_linear=1e-5)
        taken = {id(p) for mod in tables for p in mod.parameters()}
        dopt = torch.optim.Adam([p for p in m.parameters() if id(p) not in taken], lr=1e-3)
        seen = [0.0]

        def step(i):
            X, y = batches[i % N_BATCHES]
            pred = torch.sigmoid(m._logit(X)).squeeze(1)
            total = F.binary_cross_entropy(pred, y, reduction='sum') + m.regularization_loss() + m.aux_loss
            seen[0] += total.item()
            dopt.zero_grad(set_to_none=True)
            total.backward()
            topt.step()
            dopt.step()
        return step

    def head_model(kind):
        m = model_of(kind)
        m.compile(torch.optim.Adam(m.parameters(), lr=1e-3), ["binary_crossentropy"] * SCENARIOS if kind == "MMOE" else "binary_crossentropy")
        m.train()
        epoch = torch.zeros((), dtype=torch.float64, device=DEV)

        def step(i):
            X, y = batches[i % N_BATCHES]
            total, _ = m.train_step(X, y)
            epoch.add_(total.sum())
        return step

    rows = sum(vocab.values())
    lines = [f"device {torch.cuda.get_device_name(0)}; kernel sources sha256 {N.source_hash()[:16]}",
             f"{len(cols)} fields, {rows} rows in all, D = {D}, B = {B}, {N_BATCHES} batches in turn; l2 = 1e-5; one training step, per step "
             f"over {steps} steps"]
    for kind in ("WDL", "MMOE"):
        t = alternating_us([hand_written(kind), head_model(kind)], rounds, steps)
        lines.append(f"{kind} (a) hand-written loop, torch sigmoid + BCE, .item() per step: {fmt(t[0])}")
        lines.append(f"{kind} (b) HeadModel.train_step, PointLoss, regulariser tracked:     {fmt(t[1])}")
        lines.append(verdict(f"{kind} (b)", t[1], f"{kind} (a)", t[0]))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "models_time.txt"))
    ap.add_argument("--note", default=None, help="a line recorded with the measurements")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.child:
        run(a.rounds, a.steps)
        return
    text = [f"tools/models_time.py; device events around {a.steps} steps, median (min - max) per step of {a.rounds} alternating rounds"]
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
