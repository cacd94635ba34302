"""VarLenSparseFeat on the CPU side: construction, column layout, argument checks, input packing, and the pooling
restatement of tests/varlen_reference.py against torch autograd (no GPU needed)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from satrans_amd.inputs import SparseFeat, VarLenSparseFeat
from tests import varlen_reference as V


def test_construction_draws_sparse_then_varlen_tables():
    """deepctr's create_embedding_matrix order (sparse, then varlen; N(0,1) at creation, then N(0, init_std)): the
    embedding_dict tables of a varlen model come out of the same generator draws."""
    model = V.build("cpu", ("sum", "max"))
    torch.manual_seed(1021)
    cols = V.columns(("sum", "max"))
    feats = [c for c in cols if isinstance(c, SparseFeat)] + [c for c in cols if isinstance(c, VarLenSparseFeat)]
    tables = [nn.Embedding(c.vocabulary_size, c.embedding_dim) for c in feats]
    for t in tables:
        nn.init.normal_(t.weight, mean=0, std=0.0001)
    for c, t in zip(feats, tables):
        assert torch.equal(model.embedding_dict[c.embedding_name].weight.detach(), t.weight.detach()), c.name
    assert list(model.embedding_dict.keys()) == [c.embedding_name for c in feats]
    # the same seed gives the same state_dict, bit for bit
    again = V.build("cpu", ("sum", "max"))
    for k, v in model.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k


def test_feature_index_spans_and_dnn_linear_size():
    model = V.build("cpu", ("mean", "max"), length=True, dense=True, maxlen=4)
    fi = model.feature_index
    assert fi["h0"] == (5, 9) and fi["h0_len"] == (9, 10) and fi["h1"] == (10, 14) and fi["h1_len"] == (14, 15)
    assert fi["price"] == (15, 16)
    D = model.embedding_size
    assert len(model.embedding_dict) == 7
    assert tuple(model.dnn_linear.weight.shape) == (1, 7 * D + 1)            # sized by len(embedding_dict), + the dense column


def test_bad_combiner_shared_tables_and_maxlen_limit():
    from satrans_amd import SATrans

    def make(cols):
        return SATrans(cols, cols, ["dom"], [3], domain_att_layer_num=1, att_head_num=2, meta_dnn_hidden_units=(32, 16),
                       device="cpu", flag="sota")
    base = [SparseFeat("f0", 10, 16), SparseFeat("dom", 5, 16)]
    with pytest.raises(ValueError, match="combiner"):
        make(base + [VarLenSparseFeat(SparseFeat("h", 9, 16), maxlen=3, combiner="min")])
    with pytest.raises(ValueError, match="embedding tables"):
        make(base + [VarLenSparseFeat(SparseFeat("h", 10, 16, embedding_name="f0"), maxlen=3, combiner="sum")])
    with pytest.raises(ValueError, match="maxlen 33 outside 1..32"):
        make(base + [VarLenSparseFeat(SparseFeat("h", 9, 16), maxlen=33, combiner="max")])
    make(base + [VarLenSparseFeat(SparseFeat("h", 9, 16), maxlen=32, combiner="max")])       # the limit itself is accepted
    many = [SparseFeat(f"s{i}", 4, 16) for i in range(63)] + [SparseFeat("dom", 5, 16)]
    with pytest.raises(ValueError, match="at most 64"):
        make(many + [VarLenSparseFeat(SparseFeat("h", 9, 16), maxlen=3, combiner="max")])


def test_pack_and_columns_lay_out_2d_blocks():
    model = V.build("cpu", ("sum",), length=True)
    n = 4
    x = {"f0": np.arange(n), "f1": np.arange(n) % 3, "f2": np.ones(n, np.int64), "f3": np.zeros(n, np.int64),
         "dom": np.full(n, 2), "h0": np.arange(n * 3).reshape(n, 3) % 7, "h0_len": np.array([0, 1, 2, 3])}
    packed = model._pack(x)
    assert packed.shape == (n, 9)
    assert np.array_equal(packed[:, 5:8], x["h0"]) and np.array_equal(packed[:, 8], x["h0_len"])
    cols = model._columns(x)
    assert [c.shape[1] for c in cols] == [1, 1, 1, 1, 1, 3, 1]
    assert np.array_equal(np.concatenate(cols, axis=1), packed)


def _pin_cases():
    from tests import test_varlen_golden as G
    return list(G.CASES) + ["maxlen4_length"]


@pytest.mark.parametrize("name", _pin_cases())
def test_table_driven_reference_equals_the_model_restatement(name):
    """`pooled_reference` (what the direct kernel tests of tests/test_pool_kernels_gpu.py compare with) on a model's own field
    table and arena: its layer input is `layer_input`'s bit for bit - from float ids, from integer ids and from float ids with a
    fraction (`.long()` truncates) - its rows are lo + id, its mask words are `slot_mask`'s bits, and `slot_gradients` is the
    per-field autograd of `pool_rows`."""
    from tests import test_varlen_golden as G
    if name == "maxlen4_length":
        model = V.build("cpu", ("mean", "max", "sum"), maxlen=4, length=True)
        X, _ = V.batch(model, 40, seed=9)
    else:
        z, meta = G.load(name)
        model = G.build(meta, "cpu")
        X = torch.from_numpy(z["X"])
    spec, vs = V.spec_of(model)
    fields = V.pool_specs_of(model)
    arena = model.embedding_arena.detach().clone()
    D = model.embedding_size
    want = V.layer_input(V.params(model, torch.float32), X, spec, vs)
    ids = torch.ones(X.shape[1], dtype=torch.bool)                # (dense columns keep their values: they hold no ids)
    for lo, hi in spec.dense:
        ids[lo:hi] = False
    Xi = torch.where(ids, X.long().float(), X)
    forms = [X, torch.where(ids & (Xi >= 0), Xi + 0.25, Xi)] + ([X.long()] if bool(ids.all()) else [])
    for Xf in forms:
        got, rows, words = V.pooled_reference(arena, Xf, fields, D)
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert rows.dtype == torch.int32 and rows.shape == (X.shape[0], sum(f.maxlen for f in fields))
        for f in fields:
            assert torch.equal(rows[:, f.slot:f.slot + f.maxlen].long(), f.lo + X[:, f.col:f.col + f.maxlen].long())
        for f, v in zip([f for f in fields if f.varlen >= 0], vs):
            assert (f.col, f.maxlen, f.combiner, f.len_col) == (v.col, v.maxlen, v.combiner, -1 if v.len_col is None else v.len_col)
            bits = (words[:, f.varlen].unsqueeze(1) >> torch.arange(f.maxlen)) & 1
            assert torch.equal(bits.bool(), V.slot_mask(X, v)) and int(words[:, f.varlen].max()) < 2 ** f.maxlen
    dx = torch.randn(want.shape, generator=torch.Generator().manual_seed(2))
    g = V.slot_gradients(arena, X, fields, D, dx)
    n_sparse = len(spec.sparse)
    assert torch.equal(g[:, :n_sparse], dx[:, :n_sparse])
    for i, (f, v) in enumerate(zip([f for f in fields if f.varlen >= 0], vs)):
        table = model.embedding_dict[v.name].weight.detach()
        E = table[X[:, v.col:v.col + v.maxlen].long()].clone().requires_grad_(True)
        V.pool_rows(E, V.slot_mask(X, v), v).backward(dx[:, n_sparse + i])
        assert torch.equal(g[:, f.slot:f.slot + f.maxlen], E.grad)


def test_reference_max_gives_the_gradient_to_the_first_maximal_slot_at_32_slots():
    """torch.max over 32 slots (the widest list) still returns the FIRST maximal slot - what the kernel's strict `>` keeps and what
    the tests at maxlen 31 / 32 rely on: ties between neighbours, across the whole list and with every slot padding."""
    g = torch.Generator().manual_seed(4)
    v = V.VarSpec("", 0, 32, "max")
    E = torch.randn(50, 32, 32, generator=g)
    E[:10, 2] = E[:10, 1]
    E[10:20, 31] = E[10:20, 0]
    E[20:30] = E[20:30, :1]                                      # every slot equal
    valid = torch.rand(50, 32, generator=g) < 0.7
    valid[30:35] = False
    valid[35:40] = True
    E.requires_grad_(True)
    dy = torch.randn(50, 32, generator=g)
    V.pool_rows(E, valid, v).backward(dy)
    w = E.detach() - (1 - valid.float().unsqueeze(-1)) * 1e9
    top = w == w.max(1, keepdim=True)[0]
    first = top & (top.long().cumsum(1) == 1)
    assert int((top.sum(1) > 1).sum()) >= 10 * 32               # ties are there: every element of samples 20..29 at the least
    assert torch.equal(E.grad, torch.where(first, dy.unsqueeze(1), torch.zeros_like(w)))


def test_grid_constants_mirror_the_header():
    """native.GATHER_* / POOL_* are the header's SATRANS_GATHER_* / SATRANS_POOL_* (the kernels define their launch shape from those)."""
    import os
    import re
    from satrans_amd import native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "satrans_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define SATRANS_((?:GATHER|POOL)_[A-Z_]+) (\d+)\b", header)}
    for k in ("GATHER_BLOCK", "GATHER_ROWS_PER_THREAD", "GATHER_MAX_BLOCKS", "POOL_BLOCK", "POOL_ITEMS", "POOL_MAX_BLOCKS",
              "POOL_MAX_LEN", "POOL_MAX_FIELDS"):
        assert getattr(N, k) == defs[k], k
    for src, names in (("pool.hip", ("SATRANS_POOL_BLOCK", "SATRANS_POOL_ITEMS", "SATRANS_POOL_MAX_BLOCKS")),
                       ("gather.hip", ("SATRANS_GATHER_BLOCK", "SATRANS_GATHER_ROWS_PER_THREAD", "SATRANS_GATHER_MAX_BLOCKS"))):
        text = open(os.path.join(root, "satrans_amd", "csrc", src)).read()
        assert all(n in text for n in names), src


@pytest.mark.parametrize("combiner", ["sum", "mean", "max"])
@pytest.mark.parametrize("length", [False, True])
def test_reference_pooling_gradients_follow_autograd(combiner, length):
    """The backward rules the HIP kernel implements, against torch autograd of the restatement, per slot: sum -> g at valid
    slots, mean -> g / (count + 1e-8) there, max -> g at the first maximal slot of each element; 0 elsewhere."""
    model = V.build("cpu", (combiner,), length=length)
    spec, vs = V.spec_of(model)
    X, _ = V.batch(model, 64, seed=3)
    v = vs[0]
    table = model.embedding_dict["h0"].weight.detach().clone()
    table[2] = table[1]                                     # ties between slots holding ids 1 and 2
    ids = X[:, v.col:v.col + v.maxlen].long()
    E = table[ids].clone().requires_grad_(True)
    valid = V.slot_mask(X, v)
    out = V.pool_rows(E, valid, v)
    g = torch.randn_like(out)
    out.backward(g)
    if combiner == "max":
        w = E.detach() - (1 - valid.float().unsqueeze(-1)) * 1e9
        first = (w == w.max(1, keepdim=True)[0]).float().cumsum(1).eq(1) & (w == w.max(1, keepdim=True)[0])
        want = torch.where(first, g.unsqueeze(1), torch.zeros_like(E))
        assert bool((out[valid.sum(1) == 0] < -9e8).all())                  # an all-padding list pools to about -1e9
    else:
        scale = g if combiner == "sum" else g / (valid.sum(1, keepdim=True).float() + 1e-8)
        want = torch.where(valid.unsqueeze(-1), scale.unsqueeze(1), torch.zeros_like(E))
    assert torch.equal(E.grad, want)
    if combiner == "mean":
        assert bool((out[valid.sum(1) == 0] == 0).all())                    # an empty list gives 0
    # fp32 and fp64 restatements agree to fp32 rounding
    p64 = V.pool(table.double(), X.double(), v)
    assert torch.allclose(V.pool(table, X, v).double(), p64, rtol=1e-6, atol=1e-10 if combiner != "max" else 64.0)
