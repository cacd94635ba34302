"""Host side of the instance-level attention search (satrans_amd/attn_inst.py): rule construction and validation, field-name
resolution, the label / column filters against numpy, the file format, and the new C entry points without a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from satrans_amd import attn_inst as AI
from satrans_amd import native
from tests.attn_inst_reference import MATCH_DTYPE, brute_force, clauses_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["satrans_attn_inst_workspace_bytes", "satrans_attn_inst_check_rules", "satrans_attn_inst_match", "satrans_attn_inst_gather"]


def _one_rule(q=1, k=2, thr=0.2):
    return AI.resolve_rules([AI.AttentionRule([(q, k, thr)])], [f"f{i}" for i in range(8)])


def test_header_and_signatures_agree_on_the_new_symbols_and_the_abi_stays_7():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    assert native.ABI_VERSION == 7 and "#define SATRANS_ABI_VERSION 7" in header
    lib = native.lib()
    assert lib.satrans_abi_version() == 7
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in the header"
        res, args = native.SIGNATURES[name]
        assert res is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int)
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or a is ctypes.POINTER(native.AttnRule), (name, p)
                assert ("satrans_attn_rule" in p) == (a is ctypes.POINTER(native.AttnRule)), (name, p)
            else:
                assert a is (ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int), (name, p)
        assert hasattr(lib, name)
    # the struct mirrors: sizes as the header lays them out
    assert ctypes.sizeof(native.AttnAtom) == 12
    assert ctypes.sizeof(native.AttnRule) == 4 + 8 * 4 + 8 * 4 * 12
    assert ctypes.sizeof(native.AttnMatch) == 16 == AI.ATTN_MATCH_DTYPE.itemsize == MATCH_DTYPE.itemsize
    for macro, val in (("RULES", native.ATTN_MAX_RULES), ("CLAUSES", native.ATTN_MAX_CLAUSES), ("ATOMS", native.ATTN_MAX_ATOMS),
                       ("HEADS", native.ATTN_MAX_HEADS)):
        assert f"#define SATRANS_ATTN_MAX_{macro} {val}\n" in header


def test_rule_validation_in_the_library_without_a_device():
    lib = native.lib()
    good = _one_rule()
    assert lib.satrans_attn_inst_check_rules(good, 1, 8) == 0
    assert lib.satrans_attn_inst_check_rules(good, 1, 2) == -1            # k = 2 outside [0, 2)
    assert b"outside" in lib.satrans_last_error()
    assert lib.satrans_attn_inst_check_rules(None, 1, 8) == -1
    assert lib.satrans_attn_inst_check_rules(good, 0, 8) == -1
    assert lib.satrans_attn_inst_check_rules(good, 9, 8) == -1
    for field, value, word in (("n_clauses", 0, b"clauses"), ("n_clauses", 9, b"clauses")):
        bad = _one_rule()
        setattr(bad[0], field, value)
        assert lib.satrans_attn_inst_check_rules(bad, 1, 8) == -1 and word in lib.satrans_last_error()
    for n in (0, 5):
        bad = _one_rule()
        bad[0].n_atoms[0] = n
        assert lib.satrans_attn_inst_check_rules(bad, 1, 8) == -1 and b"atoms" in lib.satrans_last_error()
    for q, k in ((-1, 0), (0, -1), (8, 0), (0, 8)):
        bad = _one_rule()
        bad[0].atoms[0][0].q, bad[0].atoms[0][0].k = q, k
        assert lib.satrans_attn_inst_check_rules(bad, 1, 8) == -1 and b"outside" in lib.satrans_last_error()
    for thr in (math.nan, math.inf, -math.inf):
        bad = _one_rule()
        bad[0].atoms[0][0].thr = thr
        assert lib.satrans_attn_inst_check_rules(bad, 1, 8) == -1 and b"non-finite" in lib.satrans_last_error()
    # the launching entry points refuse the same things before any launch (the pointers are never dereferenced)
    p = ctypes.c_void_p(16)
    assert lib.satrans_attn_inst_workspace_bytes(0, 4, 19) == -1
    assert lib.satrans_attn_inst_workspace_bytes(32768, 17, 19) == -1      # H in 1..16
    assert lib.satrans_attn_inst_workspace_bytes(32768, 0, 19) == -1
    need = lib.satrans_attn_inst_workspace_bytes(32768, 4, 19)
    assert 32768 * 4 <= need <= 32768 * 4 * 2 + 4096
    assert lib.satrans_attn_inst_match(None, 16, 2, 8, good, 1, None, 0, p, 4, p, None, p, 1 << 20, None) == -1
    assert b"null pointer" in lib.satrans_last_error()
    bad = _one_rule()
    bad[0].atoms[0][0].q = 8
    assert lib.satrans_attn_inst_match(p, 16, 2, 8, bad, 1, None, 0, p, 4, p, None, p, 1 << 20, None) == -1
    assert b"outside" in lib.satrans_last_error()
    assert lib.satrans_attn_inst_match(p, 16, 2, 8, good, 1, None, 0, p, -1, p, None, p, 1 << 20, None) == -1
    assert lib.satrans_attn_inst_match(p, 16, 2, 8, good, 1, None, 0, p, 4, p, None, p, 8, None) == -4
    assert b"workspace" in lib.satrans_last_error()
    assert lib.satrans_attn_inst_gather(p, 16, 2, 8, None, 0, 4, None, 0, p, None, None, None, 0, 0, None, None) == -1
    assert lib.satrans_attn_inst_gather(p, 16, 2, 8, p, 4, 2, None, 0, p, None, None, None, 0, 0, None, None) == -1
    assert b"range" in lib.satrans_last_error()
    assert lib.satrans_attn_inst_gather(None, 16, 2, 8, p, 0, 4, None, 0, p, None, None, None, 0, 0, None, None) == -1
    assert lib.satrans_attn_inst_gather(p, 16, 2, 8, p, 0, 4, None, 0, None, None, p, None, 0, 0, None, None) == -1
    assert lib.satrans_attn_inst_gather(p, 16, 2, 8, p, 0, 4, None, 0, None, None, None, p, 4, 8, p, None) == -1
    assert b"row size" in lib.satrans_last_error()
    assert lib.satrans_attn_inst_gather(p, 16, 2, 8, p, 3, 3, None, 0, p, None, None, None, 0, 0, None, None) == 0   # empty range


def test_rule_objects_validate_their_shape():
    r = AI.AttentionRule((3, 4, 0.5))                                     # one atom
    assert r.clauses == [[(3, 4, 0.5)]]
    r = AI.AttentionRule([(15, 7, 0.2), [(15, 5, 0.2), (15, 8, 0.2)]], label=1, where=[("price", ">", 12000)])
    assert [len(c) for c in r.clauses] == [1, 2] and r.label == 1
    with pytest.raises(ValueError):
        AI.AttentionRule([])
    with pytest.raises(ValueError):
        AI.AttentionRule([(0, 1, 0.1)] * 9)
    with pytest.raises(ValueError):
        AI.AttentionRule([[(0, 1, 0.1)] * 5])
    with pytest.raises(ValueError):
        AI.AttentionRule([(0, 1, float("nan"))])
    with pytest.raises(ValueError):
        AI.AttentionRule([(0, 1, float("inf"))])
    with pytest.raises(ValueError):
        AI.AttentionRule([(0, 1, 0.1)], where=[("price", "~", 3)])
    with pytest.raises(ValueError):
        AI.resolve_rules([], ["a", "b"])
    with pytest.raises(ValueError):
        AI.resolve_rules([AI.AttentionRule((0, 1, 0.1))] * 9, ["a", "b"])
    with pytest.raises(ValueError):
        AI.resolve_rules([[(0, 1, 0.1)]], ["a", "b"])                     # not an AttentionRule


def test_field_names_resolve_against_the_layer_field_order():
    names = ["user", "item", "dom", "hist"]
    arr = AI.resolve_rules([AI.AttentionRule([("dom", "user", 0.25), [("hist", 1, 0.5), (np.int64(3), "item", 0.75)]])], names)
    r = arr[0]
    assert r.n_clauses == 2 and list(r.n_atoms)[:2] == [1, 2]
    assert (r.atoms[0][0].q, r.atoms[0][0].k, r.atoms[0][0].thr) == (2, 0, 0.25)
    assert (r.atoms[1][0].q, r.atoms[1][0].k) == (3, 1) and (r.atoms[1][1].q, r.atoms[1][1].k) == (3, 1)
    with pytest.raises(ValueError, match="price"):
        AI.resolve_rules([AI.AttentionRule(("price", 0, 0.1))], names)
    for bad in (4, -1, 1.5, True):
        with pytest.raises(ValueError):
            AI.resolve_rules([AI.AttentionRule((bad, 0, 0.1))], names)


def test_layer_field_names_put_the_pooled_varlen_fields_last():
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat

    class M:
        dnn_feature_columns = [SparseFeat("a", 4, embedding_dim=8), VarLenSparseFeat(SparseFeat("h", 9, embedding_dim=8), maxlen=3),
                               DenseFeat("price", 1), SparseFeat("b", 5, embedding_dim=8)]
    assert AI.layer_field_names(M) == ["a", "b", "h"]


@pytest.mark.parametrize("as_torch", [False, True])
def test_label_and_column_filters_against_numpy(as_torch):
    rng = np.random.default_rng(3)
    B = 500
    x = np.stack([rng.integers(0, 5, B), rng.integers(0, 20000, B), rng.random(B) * 4], axis=1).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float64)
    fi = {"pvalue": (0, 1), "price": (1, 2), "score": (2, 3)}
    rules = [AI.AttentionRule((0, 1, 0.2), label=1, where=[("pvalue", "==", 3), ("price", ">", 10000), ("pvalue", ">=", 2)]),
             AI.AttentionRule((0, 1, 0.2), where=[("price", "<=", 12000), ("score", "<", 2.5), ("pvalue", "!=", 0)]),
             AI.AttentionRule((0, 1, 0.2)),
             AI.AttentionRule((0, 1, 0.2), label=0)]
    want = np.zeros(B, dtype=np.uint8)
    want |= ((y == 1) & (x[:, 0] == 3) & (x[:, 1] > 10000) & (x[:, 0] >= 2)).astype(np.uint8) << 0
    want |= ((x[:, 1] <= 12000) & (x[:, 2] < 2.5) & (x[:, 0] != 0)).astype(np.uint8) << 1
    want |= np.uint8(1 << 2)
    want |= (y == 0).astype(np.uint8) << 3
    if as_torch:
        got = AI.eligibility(rules, torch.from_numpy(x), torch.from_numpy(y), fi)
        assert got.dtype == torch.uint8
        got = got.numpy()
    else:
        got = AI.eligibility(rules, x, y, fi)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert 0 < (want & 1).sum() < B and 0 < (want & 2).sum() < B
    with pytest.raises(ValueError, match="labels"):
        AI.eligibility(rules, x, None, fi)
    with pytest.raises(ValueError, match="colour"):
        AI.eligibility([AI.AttentionRule((0, 1, 0.2), where=[("colour", "==", 1)])], x, y, fi)


def test_brute_force_orders_by_sample_head_rule_and_masks():
    att = np.zeros((2, 3, 2, 2), dtype=np.float32)
    att[1, 0, 0, 1] = 0.9
    att[0, 2, 0, 1] = 0.9
    att[0, 2, 1, 0] = np.nan
    rules = [[[(0, 1, 0.5)]], [[(0, 1, 0.9)]], [[(0, 1, 0.1)], [(1, 0, 0.0), (0, 1, 0.8)]]]
    rec = brute_force(att, rules, first_index=10)
    assert rec.tolist() == [(10, 1, 0), (10, 1, 2), (12, 0, 0), (12, 0, 2)]      # rule 1: 0.9 > 0.9 is false; the NaN atom too
    rec = brute_force(att, rules, eligible=np.array([4, 255, 1], dtype=np.uint8))
    assert rec.tolist() == [(0, 1, 2), (2, 0, 0)]
    assert clauses_of(AI.AttentionRule([(1, 0, 0.5), [(0, 1, 0.25)]])) == [[(1, 0, 0.5)], [(0, 1, 0.25)]]


def test_file_format_and_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    M, F, C = 5, 3, 4
    result = {"index": np.array([3, 3, 70000000000, 9, 12], dtype=np.int64), "head": np.array([0, 1, 2, 3, 0], dtype=np.int32),
              "rule": np.array([0, 1, 0, 7, -1], dtype=np.int32), "pred": rng.random(M).astype(np.float32).astype(np.float64),
              "label": np.array([1.0, 0.0, 1.0, 0.0, 1.0]), "attention": rng.random((M, F, F)).astype(np.float32),
              "x": rng.integers(0, 1 << 20, (M, C)).astype(np.float32), "total": M, "truncated": False}
    path = str(tmp_path / "inst_attn_sota-showattn-instattn.txt")
    AI.write_instances(path, result)
    lines = open(path).read().split("\n")
    assert len(lines) == 3 * M + 1 and lines[-1] == ""
    assert lines[0] == f"score {result['pred'][0]},label 1.0,rule 0,head 0,index 3"
    assert lines[6] == f"score {result['pred'][2]},label 1.0,rule 0,head 2,index 70000000000"
    # the reference's lines (meta_basemodel.py:471-480): str() of every value of .tolist(), comma-joined, a trailing comma
    assert lines[1] == ",".join(str(v) for v in result["attention"][0].reshape(-1).tolist()) + ","
    assert lines[2] == ",".join(str(v) for v in result["x"][0].tolist()) + ","
    assert lines[1].count(",") == F * F and lines[2].count(",") == C
    back = AI.read_instances(path)
    for k in ("index", "head", "rule", "pred", "label"):
        assert np.array_equal(back[k], result[k]), k
    assert back["attention"].dtype == np.float32
    assert np.array_equal(back["attention"].view(np.uint32), result["attention"].reshape(M, -1).view(np.uint32))
    assert np.array_equal(back["x"], result["x"].astype(np.float64))
    # without labels the label prints as nan; no matches: an empty file
    del result["label"]
    AI.write_instances(path, result)
    assert open(path).readline().startswith(f"score {result['pred'][0]},label nan,rule 0,")
    AI.write_instances(path, {k: v[:0] if isinstance(v, np.ndarray) else v for k, v in result.items()})
    assert open(path).read() == "" and len(AI.read_instances(path)["index"]) == 0


def test_hand_records_list_every_head_of_every_sample():
    rec = AI.hand_records([7, 2, 7], 3)
    assert rec.dtype == np.int64 and rec.shape == (9, 2)
    r = np.ascontiguousarray(rec).view(MATCH_DTYPE).reshape(-1)
    assert r["index"].tolist() == [7, 7, 7, 2, 2, 2, 7, 7, 7] and r["head"].tolist() == [0, 1, 2] * 3 and (r["rule"] == -1).all()


def test_the_reference_rules_example_resolves_on_the_alimama_fields():
    import importlib.util
    from tests.helpers import Case
    spec = importlib.util.spec_from_file_location("alimama_instattn", os.path.join(ROOT, "examples", "alimama_instattn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fields = Case("alimama_sota_pos").meta["fields"]
    rules = mod.alimama_rules()
    arr = AI.resolve_rules(rules, fields)
    assert [arr[0].n_clauses, arr[1].n_clauses] == [2, 2] and list(arr[1].n_atoms)[:2] == [1, 2]     # A and B; A and (B or C)
    assert (arr[0].atoms[0][0].q, arr[0].atoms[0][0].k) == (7, 5) and arr[1].atoms[0][0].k == 7
    assert (arr[1].atoms[1][0].k, arr[1].atoms[1][1].k) == (5, 8)
    assert all(r.label == 1 and ("pvalue_level", "==", 3) in r.where for r in rules)
