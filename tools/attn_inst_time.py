"""Cost of the instance-level attention search (attention_instances / predict's 'instattn', csrc/attn_inst.hip) at the AliCCP shape
(19 fields, 4 heads) and the prediction batch of 32,768 samples, two rules of four atoms each (`A and B and (C or D)`), medians
of `--reps` repetitions (CUDA events around the calls):
  - the match call (count, scan, write kernels) on one layer's attention [H, 32768, F, F] with thresholds at the 0.5 quantile
    of each atom (every atom is read by many lanes: the search's worst case) and at the 0.97 quantile (few matches);
  - the gather of the matches (maps, rows) and of their probabilities;
  - beside them, at the same shape: one statistics call on the same buffer (tools/attn_stats_time.py; its block kernel reads
    the whole map once), and what instance-level attention cost before the search existed: a capture_attention forward, the
    device-to-host copy of [H, B, F, F] and the numpy matcher (tests/attn_inst_reference.py) on the copy.
Per-kernel dispatch times: `rocprofv3 --kernel-trace --stats -- python tools/attn_inst_time.py`.
Usage: python tools/attn_inst_time.py [--reps 9] [--out profiles/attn_inst_time.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from satrans_amd import attn_inst as AI  # noqa: E402
from satrans_amd import attn_stats as AS  # noqa: E402
from satrans_amd import native  # noqa: E402
from tests.attn_inst_reference import brute_force, clauses_of  # noqa: E402

B = 32768
ATOMS = [[(7, 5), (7, 15), (3, 3), (12, 1)], [(15, 7), (2, 9), (15, 5), (15, 8)]]      # rule r: a0 and a1 and (a2 or a3)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def events_us(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_inst_time.txt"))
    a = ap.parse_args()
    reps = max(7, a.reps)
    cfg = bench.make_config("aliccp")
    X, _ = bench.synth_batches(B, 3, cfg=cfg)
    y = (np.random.RandomState(4).rand(B) < 0.3).astype(np.float64)
    dom = X[:, cfg["fields"].index(cfg["domain"])].astype(np.int64)
    model = bench.build_model("cuda:0", 0.005, cfg=cfg)
    eng = model._require_engine()
    model.eval()
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    res = dict(config="aliccp", F=eng.F, H=eng.H, batch=B, reps=reps, source_hash=native.source_hash()[:16])

    # what the parent offers: capture_attention, the whole [H, B, F, F] through the host, the numpy matcher
    def capture():
        eng.forward(Xd, training=False, capture_attention=True)
        return model.domain_int_layers[0].normalized_att_scores
    capture()
    torch.cuda.synchronize()
    t_fwd, t_copy, t_np = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        att = capture()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        att_h = att.cpu().numpy()
        t2 = time.perf_counter()
        t_fwd.append(1e6 * (t1 - t0))
        t_copy.append(1e6 * (t2 - t1))
    res["capture_forward_us"], res["capture_copy_to_host_us"] = median(t_fwd), median(t_copy)
    res["attention_MB"] = att.numel() * 4 / 1e6

    for label, quant in (("q50", 0.5), ("q97", 0.97)):
        rules = [AI.AttentionRule([(q0[0], q0[1], float(np.quantile(att_h[:, :, q0[0], q0[1]], quant))),
                                   (q1[0], q1[1], float(np.quantile(att_h[:, :, q1[0], q1[1]], quant))),
                                   [(q2[0], q2[1], float(np.quantile(att_h[:, :, q2[0], q2[1]], quant))),
                                    (q3[0], q3[1], float(np.quantile(att_h[:, :, q3[0], q3[1]], quant)))]])
                 for q0, q1, q2, q3 in ATOMS]
        plain = [clauses_of(r) for r in rules]
        for _ in range(reps):
            t0 = time.perf_counter()
            want = brute_force(att_h, plain)
            t_np.append(1e6 * (time.perf_counter() - t0))
        ctx = AI.AttentionInstances(eng, AI.resolve_rules(rules, AI.layer_field_names(model)), 0, 65536)
        ctx.set_batch(0)
        ctx._x_view(Xd)
        lib = eng.lib
        need = int(lib.satrans_attn_inst_workspace_bytes(B, eng.H, eng.F))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")

        def match():
            native.check(lib.satrans_attn_inst_match(att.data_ptr(), B, eng.H, eng.F, ctx.rules, ctx.n_rules, None, 0,
                                                     ctx.records.data_ptr(), ctx.capacity, ctx.total.data_ptr(),
                                                     ctx._range.data_ptr(), ws.data_ptr(), need, st), "match")

        def gather():
            native.check(lib.satrans_attn_inst_gather(att.data_ptr(), B, eng.H, eng.F, ctx.records.data_ptr(), 0, ctx.capacity,
                                                      ctx._range.data_ptr(), 0, ctx.maps.data_ptr(), eng._ws[B]["prob"].data_ptr(),
                                                      ctx.pred.data_ptr(), Xd.data_ptr(), Xd.stride(0), Xd.shape[1],
                                                      ctx.x_rows.data_ptr(), st), "gather")
        match()
        gather()
        res[f"{label}_matches"] = int(ctx.total.item())
        assert res[f"{label}_matches"] == len(want)
        res[f"{label}_match_call_us"] = events_us(match, reps, before=ctx.total.zero_)
        res[f"{label}_gather_us"] = events_us(gather, reps)
        res[f"{label}_numpy_matcher_us"] = median(t_np[-reps:])

    # one statistics call on the same buffer
    S = cfg["n_domains"]
    sctx = AS.AttentionStatistics(eng, S)
    sctx.set_batch(torch.from_numpy(AS.class_keys(dom, y, S, AS.scenario_bias(dom))).cuda())
    sctx.accumulate(0, att, B, st)
    res["stats_call_us"] = events_us(lambda: sctx.accumulate(0, att, B, st), reps)
    res["plain_forward_us"] = events_us(lambda: eng.forward(Xd, training=False), reps)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
