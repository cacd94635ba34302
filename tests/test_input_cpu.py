"""LinearModel and FeatureEmbedding without a GPU: the fp64 restatement against the reference's recorded runs, the premise of
the GPU bounds, the max-pooling draws, the modules' construction and state, the C ABI's new symbols and their argument
validation."""
import ctypes
import os
import re

import pytest
import torch

from satrans_amd import native
from satrans_amd.basemodel import _LinearTables, make_embedding_tables
from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features
from tests import input_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("satrans_linear_workspace_bytes", "satrans_linear_fwd", "satrans_linear_bwd")
OUT_BOUND, GRAD_REL, GRAD_ABS = R.OUT_BOUND, R.GRAD_REL, R.GRAD_ABS


def within_out(got, want):
    """2e-5 max|.|; and, where a batch holds an all-padding max list (about -1e9), the same on the other samples by themselves."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= OUT_BOUND * float(want.abs().max())
    small = want.abs().flatten(1).max(1)[0] < 1e8
    if bool(small.any()) and not bool(small.all()):
        assert float((got[small] - want[small]).abs().max()) <= OUT_BOUND * float(want[small].abs().max())


def within_grad(got, want, what=""):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    assert float((got - want).abs().max()) <= GRAD_REL * float(want.abs().max()) + GRAD_ABS, what


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_every_fixture(name):
    """The recorded side is the reference's fp32 run, the restatement fp64 on the same fp32 inputs: within the sibling bounds;
    what is copied (the embeddings of sparse fields, the dense values) agrees exactly."""
    fx = R.load_golden(name)
    cols = R.columns_from_fixture(fx)
    fi = build_input_features(cols)
    spec = R.spec_of(cols, fi)
    X = torch.from_numpy(fx["X"])
    assert X.shape == (24, max(hi for _, hi in fi.values()))
    Pl, Pe = R.fixture_params(fx, "linear"), R.fixture_params(fx, "emb")
    logit, emb, gl, ge = R.loss_and_grads(Pl, Pe, X, spec, torch.from_numpy(fx["c"]), torch.from_numpy(fx["C"]), torch.float64)
    within_out(logit, torch.from_numpy(fx["out/linear_logit"]))
    within_out(emb, torch.from_numpy(fx["out/emb"]))
    ns = len(spec.sparse)
    assert torch.equal(emb[:, :ns].float(), torch.from_numpy(fx["out/emb"])[:, :ns])
    assert torch.equal(R.dense_values(X, spec), torch.from_numpy(fx["out/dense"]))
    assert sorted(gl) == sorted(R.fixture_params(fx, "grad_linear")) and sorted(ge) == sorted(R.fixture_params(fx, "grad_emb"))
    for k, g in gl.items():
        within_grad(g, torch.from_numpy(fx[f"grad_linear/{k}"]), k)
    for k, g in ge.items():
        within_grad(g, torch.from_numpy(fx[f"grad_emb/{k}"]), k)
    if name == "varlen":      # the two special samples are there
        v = dict((n, s) for n, s in spec.varlen)
        assert int(R.V.slot_mask(X, v["h_mean"])[3].sum()) == 0 and int(R.V.slot_mask(X, v["h_max"])[5].sum()) == 0
        assert float(fx["out/linear_logit"][5, 0]) < -9e8 and bool((fx["out/emb"][3, ns + 1] == 0).all())
    if name == "shared":
        assert list(fx["col/embedding_name"]).count("item") == 2 and "emb/embedding_dict.item.weight" in fx


def _draws():
    return [(c.name, lambda c=c: R.draw_case(c)[1:]) for c in R.SWEEP] + \
           [(f"skew_d{D}", lambda D=D: R.draw_skew(8269, D)[1:]) for D in (16, 128)]


@pytest.mark.parametrize("name,make", _draws(), ids=[n for n, _ in _draws()])
def test_premise_of_the_gpu_bounds(name, make):
    """The GPU tests hold the modules to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients against the
    fp64 restatement.  On every draw they use, torch's own fp32 run of the literal form under autograd stays within a quarter of
    those bounds (measured worst over the draws: results 1.2e-2 of their bound at B = 8269, F = 19; gradients 4.0e-2 of theirs in
    the skew case at D = 128, where one row sums all 8269 samples)."""
    fi, spec, X, Pl, Pe, c, Cw = make()
    want = R.loss_and_grads(Pl, Pe, X, spec, c, Cw, torch.float64)
    got = R.loss_and_grads(Pl, Pe, X, spec, c, Cw, torch.float32)
    worst_out = worst_grad = 0.0
    for g, w in zip(got[:2], want[:2]):
        if w is not None and float(w.abs().max()) > 0:
            worst_out = max(worst_out, float((g.double() - w).abs().max()) / (OUT_BOUND * float(w.abs().max())))
    for gd, wd in zip(got[2:], want[2:]):
        for k in wd:
            bound = GRAD_REL * float(wd[k].abs().max()) + GRAD_ABS
            worst_grad = max(worst_grad, float((gd[k].double() - wd[k]).abs().max()) / bound)
    print(f"[input-premise] {name}: results {worst_out:.2e} of their bound, gradients {worst_grad:.2e} of theirs")
    assert worst_out <= 0.25 and worst_grad <= 0.25


def test_max_pooling_draws_have_no_tie_among_valid_slots():
    """The gradient of a max is undefined at a tie: no draw of the sweep, the skew case or the fixtures has one among VALID
    slots, counted from the restatement alone (`draw` redraws until that holds).  No case is left out."""
    n_max = 0
    for name, make in _draws():
        fi, spec, X, Pl, Pe, _c, _C = make()
        n_max += sum(v.combiner == "max" for _, v in spec.varlen)
        assert R.max_ties(Pl, X, spec) == 0 and R.max_ties(Pe, X, spec) == 0, name
    for name in R.GOLDEN_CASES:
        fx = R.load_golden(name)
        cols = R.columns_from_fixture(fx)
        spec = R.spec_of(cols, build_input_features(cols))
        X = torch.from_numpy(fx["X"])
        n_max += sum(v.combiner == "max" for _, v in spec.varlen)
        assert R.max_ties(R.fixture_params(fx, "linear"), X, spec) == 0 and R.max_ties(R.fixture_params(fx, "emb"), X, spec) == 0, name
    assert n_max >= 10
    # the counter sees a tie when there is one
    cols = [VarLenSparseFeat(SparseFeat("h", 5, embedding_dim=16), maxlen=2, combiner="max")]
    spec = R.spec_of(cols, build_input_features(cols))
    P = {R.key("h"): torch.tensor([[0.0], [1.0], [1.0], [2.0], [3.0]])}
    assert R.max_ties(P, torch.tensor([[1.0, 2.0], [1.0, 3.0], [0.0, 0.0]]), spec) == 1


def _golden_columns(name):
    fx = R.load_golden(name)
    cols = R.columns_from_fixture(fx)
    return fx, cols, build_input_features(cols)


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_construction_draws_keys_and_round_trip(name):
    from satrans_amd import FeatureEmbedding, LinearModel
    fx, cols, fi = _golden_columns(name)
    torch.manual_seed(77)
    lin = LinearModel(cols, fi, init_std=0.01)
    torch.manual_seed(77)
    ref = _LinearTables(cols, 0.01)
    assert list(lin.state_dict()) == list(ref.state_dict()) == [k[len("linear/"):] for k in fx if k.startswith("linear/")]
    for k, v in ref.state_dict().items():
        assert torch.equal(lin.state_dict()[k], v), k
        assert tuple(v.shape) == fx[f"linear/{k}"].shape
    torch.manual_seed(78)
    fe = FeatureEmbedding(cols, fi, init_std=0.01)
    torch.manual_seed(78)
    tables = make_embedding_tables(cols, 0.01)
    want = {f"embedding_dict.{k}": v for k, v in tables.state_dict().items()}
    assert list(fe.state_dict()) == list(want) == [k[len("emb/"):] for k in fx if k.startswith("emb/")]
    for k, v in want.items():
        assert torch.equal(fe.state_dict()[k], v), k
    # the tables are views of one arena, in arena order, and stay so through load_state_dict and a dtype round trip
    for mod, prefix, width in ((lin, "linear", 1), (fe, "emb", 16)):
        mod.load_state_dict(R.fixture_params(fx, prefix))
        for k, v in R.fixture_params(fx, prefix).items():
            assert torch.equal(mod.state_dict()[k], v), k
        assert mod.arena.shape == (sum(t.weight.shape[0] for t in mod.embedding_dict.values()), width)
        for trip in range(2):
            at = 0
            for n in mod._layout.names:
                w = mod.embedding_dict[n].weight
                assert w.data_ptr() == mod.arena.data_ptr() + at * width * 4 and mod._layout.table_rows[n] == (at, w.shape[0])
                at += w.shape[0]
            mod.double().float()      # `_apply` rebuilds the arena
        assert all(p.requires_grad and p.is_leaf for p in mod.parameters())
    if name == "shared":      # two fields, one embedding_name: one parameter, one span of the arena
        assert [n for n, _ in fe.named_parameters()] == ["embedding_dict.user.weight", "embedding_dict.item.weight"]
        f = fe._layout.fields
        assert (f[1].lo, f[1].hi) == (f[2].lo, f[2].hi) == (50, 81) and f[1].col != f[2].col
        f = lin._layout.fields
        assert (f[1].lo, f[1].hi) == (f[2].lo, f[2].hi) == (50, 81)
    if name == "plain":
        assert lin._layout.dense_cols == [1, 4, 5, 6] and lin.weight.shape == (4, 1)


def test_modules_without_tables_or_without_dense():
    from satrans_amd import LinearModel
    dense_only = [DenseFeat("a", 2), DenseFeat("b", 1)]
    m = LinearModel(dense_only, build_input_features(dense_only))
    assert list(m.state_dict()) == ["weight"] and m.arena is None and m._layout.F == 0
    sparse_only = [SparseFeat("s", 7, embedding_dim=16)]
    m = LinearModel(sparse_only, build_input_features(sparse_only))
    assert list(m.state_dict()) == ["embedding_dict.s.weight"] and not hasattr(m, "weight")
    m = LinearModel([], build_input_features(sparse_only))
    assert list(m.state_dict()) == []
    out = m(torch.ones(5, 1))      # neither: the reference's zeros, no launch
    assert out.shape == (5, 1) and float(out.abs().max()) == 0.0


def test_constructor_errors_fire_before_any_launch():
    from satrans_amd import FeatureEmbedding, LinearModel
    ok = [SparseFeat("s", 7, embedding_dim=16), DenseFeat("d", 1)]

    def fe(cols):
        return FeatureEmbedding(cols, build_input_features(cols))

    def lm(cols):
        return LinearModel(cols, build_input_features(cols))

    for bad_d in (8, 4, 48, 256):
        with pytest.raises(ValueError, match=r"\{16, 32, 64, 128\}"):
            fe([SparseFeat("s", 7, embedding_dim=bad_d)])
    with pytest.raises(ValueError, match=r"\{16, 32, 64, 128\}"):
        fe([SparseFeat("s", 7, embedding_dim=16), SparseFeat("t", 7, embedding_dim=32)])
    lm([SparseFeat("s", 7, embedding_dim=8)])      # the linear tables are 1 wide whatever embedding_dim says
    many = [SparseFeat(f"s{i}", 3, embedding_dim=16) for i in range(native.POOL_MAX_FIELDS + 1)]
    long_list = [VarLenSparseFeat(SparseFeat("h", 50, embedding_dim=16), maxlen=native.POOL_MAX_LEN + 1, combiner="sum")]
    odd = [VarLenSparseFeat(SparseFeat("h", 50, embedding_dim=16), maxlen=3, combiner="median")]
    for make in (fe, lm):
        with pytest.raises(ValueError, match="POOL_MAX_FIELDS"):
            make(many)
        with pytest.raises(ValueError, match="POOL_MAX_LEN"):
            make(long_list)
        with pytest.raises(ValueError, match="combiner"):
            make(odd)
        make(many[:-1])
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError):
        lm(many)
    assert torch.equal(torch.random.get_rng_state(), state)      # refused before a generator draw
    with pytest.raises(ValueError, match="no SparseFeat"):
        fe([DenseFeat("d", 1)])
    with pytest.raises(ValueError, match="feature_index"):
        LinearModel(ok, build_input_features(ok[:1]))
    m, e = lm(ok), fe(ok)
    with pytest.raises(NotImplementedError, match="sparse_feat_refine_weight"):
        m(torch.zeros(3, 2), sparse_feat_refine_weight=torch.ones(3, 1))
    for mod in (m, e):
        with pytest.raises(ValueError, match="expected X"):
            mod(torch.zeros(3, 1))
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            mod(torch.zeros(3, 2))


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    assert ctypes.sizeof(native.LinearDesc) == 6 * 4 + 3 * 8 + 6 * 8
    body = re.search(r"typedef struct satrans_linear_desc \{(.*?)\} satrans_linear_desc;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in native.LinearDesc._fields_], names
    for macro, value in (("SAMPLES", native.LINEAR_SAMPLES), ("MAX_BLOCKS", native.LINEAR_MAX_BLOCKS),
                         ("SEG_CHUNK", native.LINEAR_SEG_CHUNK), ("DW_ROW_CHUNK", native.LINEAR_DW_ROW_CHUNK)):
        assert int(re.search(r"#define SATRANS_LINEAR_%s (\d+)" % macro, header).group(1)) == value


def linear_desc(B=4, fields=((0, 1, 0, -1, 0, -1, 0, 10),), R=None, Fv=None, n_dense=0, x_stride=8, arena_rows=10, id_dtype=0,
                dense_stride=8):
    """fields: tuples in satrans_pool_field's member order.  The pointers stay NULL; `keep` holds the host array alive."""
    d = native.LinearDesc()
    arr = (native.PoolField * max(1, len(fields)))()
    for i, t in enumerate(fields):
        (arr[i].col, arr[i].maxlen, arr[i].combiner, arr[i].len_col, arr[i].slot, arr[i].varlen, arr[i].lo, arr[i].hi) = t
    d.B, d.F, d.n_dense, d.id_dtype = B, len(fields), n_dense, id_dtype
    d.R = sum(t[1] for t in fields) if R is None else R
    d.Fv = sum(t[5] >= 0 for t in fields) if Fv is None else Fv
    d.x_stride, d.arena_rows, d.dense_stride = x_stride, arena_rows, dense_stride
    d.fields = ctypes.cast(arr, ctypes.POINTER(native.PoolField)) if fields else None
    d.keep = arr
    return d


def test_library_validates_descriptors_without_a_device():
    lib, by = native.lib(), ctypes.byref
    null = ctypes.POINTER(native.LinearDesc)()
    err = lib.satrans_last_error

    def refused(d, code, text):
        assert lib.satrans_linear_workspace_bytes(by(d)) == code and text in err(), (text, err())
        assert lib.satrans_linear_fwd(by(d), None, None, None, None, None, None) == code and text in err(), (text, err())
        assert lib.satrans_linear_bwd(by(d), None, None, None, None, None, None, None, None, None, None) == code and text in err()

    assert lib.satrans_linear_workspace_bytes(null) == -1 and b"null descriptor" in err()
    assert lib.satrans_linear_fwd(null, None, None, None, None, None, None) == -1
    assert lib.satrans_linear_bwd(null, None, None, None, None, None, None, None, None, None, None) == -1
    for kw in (dict(B=0), dict(B=-3), dict(n_dense=-1), dict(x_stride=-1), dict(arena_rows=-5), dict(dense_stride=-2)):
        refused(linear_desc(**kw), -1, b"bad sizes")
    refused(linear_desc(fields=(), n_dense=0), -1, b"neither fields nor dense")
    refused(linear_desc(fields=(), R=3, n_dense=2), -1, b"without fields")
    refused(linear_desc(id_dtype=3), -1, b"id_dtype")
    many = tuple((i % 8, 1, 0, -1, i, -1, 0, 10) for i in range(native.POOL_MAX_FIELDS + 1))
    refused(linear_desc(fields=many), -1, b"fields)")
    refused(linear_desc(fields=((0, native.POOL_MAX_LEN + 1, 1, -1, 0, 0, 0, 10),), x_stride=64), -2, b"maxlen")
    refused(linear_desc(fields=((0, 2, 0, -1, 0, -1, 0, 10),)), -2, b"maxlen")              # a SparseFeat is one slot
    refused(linear_desc(fields=((0, 3, 4, -1, 0, 0, 0, 10),)), -1, b"combiner")
    refused(linear_desc(fields=((6, 3, 1, -1, 0, 0, 0, 10),)), -1, b"X columns")             # columns 6..8 of a row of 8
    refused(linear_desc(fields=((0, 3, 1, 8, 0, 0, 0, 10),)), -1, b"X columns")              # the length column
    refused(linear_desc(fields=((0, 1, 0, -1, 0, -1, 4, 11),)), -1, b"outside the arena")
    refused(linear_desc(fields=((0, 1, 0, -1, 0, -1, 5, 5),)), -1, b"outside the arena")
    refused(linear_desc(fields=((0, 1, 0, -1, 1, -1, 0, 10),)), -1, b"first slot")
    refused(linear_desc(R=2), -1, b"the fields give")
    refused(linear_desc(B=2 ** 30, fields=((0, 1, 0, -1, 0, -1, 0, 10), (1, 3, 1, -1, 1, 0, 0, 10))), -1, b"31 bits")
    # a good descriptor: the workspace is [B R] contributions, two partials per chunk of the sorted list, the dweight partials
    d = linear_desc(B=300, fields=((0, 1, 0, -1, 0, -1, 0, 10), (1, 3, 3, 4, 1, 0, 0, 10)), n_dense=5)
    n, up = 300 * 4, lambda x: (x + 255) // 256 * 256
    chunks = -(-n // native.LINEAR_SEG_CHUNK)
    assert lib.satrans_linear_workspace_bytes(by(d)) == \
        up(4 * n) + 2 * up(4 * chunks) + up(4 * 5 * -(-300 // native.LINEAR_DW_ROW_CHUNK))
    assert lib.satrans_linear_fwd(by(d), None, None, None, None, None, None) == -1 and b"null pointer" in err()
    assert lib.satrans_linear_bwd(by(d), None, None, None, None, None, None, None, None, None, None) == -1 and b"null pointer" in err()
    dense_only = linear_desc(fields=(), n_dense=3)
    assert lib.satrans_linear_workspace_bytes(by(dense_only)) == 256
