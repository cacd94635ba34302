"""LinearModel and FeatureEmbedding on the MI355X against the fp64 restatement of tests/input_reference.py: the sweep of shapes
and id forms, the skewed batches of the segment sum, batch independence, out-of-range ids, the lookup's exact copies, the
reference's recorded runs, and three Adam steps of a model built from the two modules and a head against its torch-ops twin."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from satrans_amd.inputs import PackedInput, build_input_features
from tests import input_reference as R
from tests import varlen_reference as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_BOUND, GRAD_REL, GRAD_ABS = R.OUT_BOUND, R.GRAD_REL, R.GRAD_ABS


_worst = {"out": 0.0, "grad": 0.0}


@pytest.fixture(autouse=True)
def report_worst_ratio(request):
    """Every test prints the largest error it saw as a share of its bound (measured figures: DESIGN.md §3.19)."""
    _worst.update(out=0.0, grad=0.0)
    yield
    print(f"[input] {request.node.name}: worst result {_worst['out']:.2e} of its bound, worst gradient {_worst['grad']:.2e} of its bound")


def within_out(got, want, what=""):
    """2e-5 max|.|; where a batch holds an all-padding max list (about -1e9), the same on the other samples by themselves too."""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, what
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    _worst["out"] = max(_worst["out"], err / (OUT_BOUND * scale))
    assert err <= OUT_BOUND * scale, (what, err, OUT_BOUND * scale)
    small = want.abs().flatten(1).max(1)[0] < 1e8
    if bool(small.any()) and not bool(small.all()):
        assert float((got[small] - want[small]).abs().max()) <= OUT_BOUND * float(want[small].abs().max()), what


def within_grad(got, want, what=""):
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, what
    err, bound = float((got - want).abs().max()), GRAD_REL * float(want.abs().max()) + GRAD_ABS
    _worst["grad"] = max(_worst["grad"], err / bound)
    assert err <= bound, (what, err, bound)


def device_input(X, spec, ids):
    """The fp32 matrix, or integer ids: a bare matrix without dense columns, PackedInput(ids, dense block) with them."""
    if ids == "f32":
        return X.to(DEV)
    Xi = X.to(torch.int32 if ids == "i32" else torch.int64).to(DEV)
    return PackedInput(Xi, X[:, spec.dense_cols].contiguous().to(DEV)) if spec.dense_cols else Xi


def linear_module(cols, fi, Pl):
    from satrans_amd import LinearModel
    m = LinearModel(cols, fi, device=DEV)
    m.load_state_dict(Pl)
    return m


def embedding_module(cols, fi, Pe):
    from satrans_amd import FeatureEmbedding
    m = FeatureEmbedding(cols, fi, device=DEV)
    m.load_state_dict(Pe)
    return m


def run_linear(mod, Xd, c):
    mod.zero_grad(set_to_none=True)
    logit = mod(Xd)
    (logit.squeeze(1) * c.to(DEV)).sum().backward()
    return logit.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in mod.named_parameters()}


def run_embedding(mod, Xd, Cw):
    mod.zero_grad(set_to_none=True)
    emb, dense = mod(Xd)
    (emb * Cw.to(DEV)).sum().backward()
    return emb.detach().cpu(), dense, {k: p.grad.detach().cpu().clone() for k, p in mod.named_parameters()}


def assert_ungathered_rows_are_zero(grads, P, X, spec):
    for k, hit in R.gathered_rows(P, X, spec).items():
        rest = grads[k][~hit]
        assert rest.numel() == 0 or (float(rest.abs().max()) == 0.0 and not bool(torch.signbit(rest).any())), k


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_linear_forward_and_backward_sweep(case):
    cols, fi, spec, X, Pl, _Pe, c, _C = R.draw_case(case)
    want_logit, _, want_g, _ = R.loss_and_grads(Pl, {}, X, spec, c, None, torch.float64)
    mod = linear_module(cols, fi, Pl)
    assert (mod._layout.F, mod._layout.n_dense) == (case.n_sparse + len(case.varlen), case.n_dense)
    logit, grads = run_linear(mod, device_input(X, spec, case.ids), c)
    within_out(logit, want_logit, f"{case.name} logit")
    assert sorted(grads) == sorted(want_g)
    for k in want_g:
        within_grad(grads[k], want_g[k], f"{case.name} {k}")
    assert_ungathered_rows_are_zero(grads, Pl, X, spec)
    if case.ids != "f32":      # the three id forms read the same ids: the same bits
        again, g2 = run_linear(mod, X.to(DEV), c)
        assert torch.equal(again, logit) and all(torch.equal(g2[k], grads[k]) for k in grads)


@pytest.fixture(scope="module")
def skew():
    """The B = 8269 skew draw at D = 16 and its fp64 gradients, computed once and left unchanged."""
    cols, fi, spec, X, Pl, Pe, c, Cw = R.draw_skew(8269, 16)
    want = R.loss_and_grads(Pl, Pe, X, spec, c, Cw, torch.float64)
    return cols, fi, spec, X, Pl, Pe, c, Cw, want


def test_linear_segment_sum_under_skew(skew):
    """One row gathered by all 8269 samples (its run crosses every chunk and workgroup bound of the segment sum), a table of one
    row, a field of distinct ids, two fields on one table: gradients within the bound, ungathered rows exactly +0.0, two runs
    bit-identical in logit, every table gradient and dweight."""
    cols, fi, spec, X, Pl, _Pe, c, _C, want = skew
    mod = linear_module(cols, fi, Pl)
    Xd = X.to(DEV)
    logit, grads = run_linear(mod, Xd, c)
    within_out(logit, want[0], "skew logit")
    for k in want[2]:
        within_grad(grads[k], want[2][k], f"skew {k}")
    hot = grads[R.key("hot")]
    assert float(hot[7].abs()) > 0 and int((hot != 0).sum()) == 1
    assert_ungathered_rows_are_zero(grads, Pl, X, spec)
    assert float(grads[R.key("wide")][[0, 1, 8269 + 2]].abs().max()) == 0.0 and float(grads[R.key("pair")][28].abs()) == 0.0
    logit2, grads2 = run_linear(mod, Xd, c)
    assert torch.equal(logit2, logit)
    for k in grads:
        assert torch.equal(grads2[k], grads[k]), k


def test_linear_logit_does_not_depend_on_the_batch():
    case = next(c for c in R.SWEEP if c.name == "b260_f64")
    cols, fi, spec, X, Pl, _Pe, _c, _C = R.draw_case(case)
    mod = linear_module(cols, fi, Pl)
    Xd = X.to(DEV)
    with torch.no_grad():
        whole = mod(Xd)
        alone = torch.cat([mod(Xd[b:b + 1]) for b in range(case.B)])
        part = mod(Xd[100:137])
    assert torch.equal(alone, whole) and torch.equal(part, whole[100:137])


def test_out_of_range_id_raises_and_the_next_call_is_clean():
    case = next(c for c in R.SWEEP if c.name == "b37_f19")
    cols, fi, spec, X, Pl, Pe, c, Cw = R.draw_case(case)
    lin, emb = linear_module(cols, fi, Pl), embedding_module(cols, fi, Pe)
    want = lin(X.to(DEV)).detach().cpu()
    first = cols[0]
    bad = X.clone()
    bad[5, fi[first.name][0]] = first.vocabulary_size
    padded = X.clone()      # a padding slot behind the length of a list is looked up too, as nn.Embedding would
    v = next(c for c in cols if getattr(c, "length_name", None) is not None)
    padded[:, fi[v.length_name][0]] = 1
    padded[9, fi[v.name][0] + 2] = v.vocabulary_size
    for mod in (lin, emb):
        for Xb in (bad, padded, -1 - bad):
            with pytest.raises(IndexError):
                mod(Xb.to(DEV))
            out = mod(X.to(DEV))      # the status word was cleared
            if mod is lin:
                assert torch.equal(out.detach().cpu(), want)


def pool_specs(mod):
    names = {0: "copy", 1: "sum", 2: "mean", 3: "max"}
    return [V.PoolSpec(f.col, f.maxlen, names[f.combiner], f.len_col, f.slot, f.varlen, f.lo, f.hi)
            for f in mod._layout.fields[:mod._layout.F]]


@pytest.mark.parametrize("name", ["b37_f19", "b260_f64", "b8269_f19", "one"])
def test_feature_embedding_forward_is_exact(name):
    """Sparse fields: bit-identical to arena[lo_f + id]; pooled fields: equal to varlen_reference.pooled_reference (fp32, slot
    order), as tests/test_varlen_gpu.py requires of the pooled gather; dense: the X columns bit for bit."""
    case = next(c for c in R.SWEEP if c.name == name)
    cols, fi, spec, X, _Pl, Pe, _c, Cw = R.draw_case(case)
    mod = embedding_module(cols, fi, Pe)
    with torch.no_grad():
        emb, dense = mod(device_input(X, spec, case.ids))
    arena = mod.arena.detach().cpu()
    for f, (n, col) in enumerate(spec.sparse):
        lo, _ = mod._layout.table_rows[n]
        assert torch.equal(emb[:, f].cpu(), arena[lo + X[:, col].long()]), n
    want, _rows, _words = V.pooled_reference(arena, X, pool_specs(mod), case.D)
    assert torch.equal(emb.cpu(), want)
    if spec.dense_cols:
        assert torch.equal(dense.cpu(), X[:, spec.dense_cols]) and not dense.requires_grad
    else:
        assert dense is None


@pytest.mark.parametrize("form", ["segment_sums", "grad_dense"])
@pytest.mark.parametrize("D", [16, 128])
def test_feature_embedding_backward_under_skew(D, form, skew):
    """Table gradients under a random d emb against fp64 (index_add of the slot gradients through autograd), with the shared
    table and the all-one-id field at B = 8269, through both kernels of the dense gradient: within the gradient bound, ungathered
    rows exactly 0, two runs bit-identical."""
    if D == 16:
        cols, fi, spec, X, _Pl, Pe, _c, Cw, want = skew
        want_g = want[3]
    else:
        cols, fi, spec, X, _Pl, Pe, c, Cw = R.draw_skew(8269, D)
        want_g = R.loss_and_grads({}, Pe, X, spec, c, Cw, torch.float64)[3]
    mod = embedding_module(cols, fi, Pe)
    assert mod.dense_gradient == "segment_sums"
    mod.dense_gradient = form
    Xd = X.to(DEV)
    emb, dense, grads = run_embedding(mod, Xd, Cw)
    assert torch.equal(dense.cpu(), X[:, spec.dense_cols])
    for k in want_g:
        within_grad(grads[k], want_g[k], f"skew D={D} {k}")
    assert_ungathered_rows_are_zero(grads, Pe, X, spec)
    _, _, grads2 = run_embedding(mod, Xd, Cw)
    for k in grads:
        assert torch.equal(grads2[k], grads[k]), k


@pytest.mark.parametrize("name", ["b37_f19", "b260_f64"])
def test_feature_embedding_backward_sweep(name):
    case = next(c for c in R.SWEEP if c.name == name)
    cols, fi, spec, X, _Pl, Pe, c, Cw = R.draw_case(case)
    want = R.loss_and_grads({}, Pe, X, spec, c, Cw, torch.float64)
    mod = embedding_module(cols, fi, Pe)
    emb, _dense, grads = run_embedding(mod, device_input(X, spec, case.ids), Cw)
    within_out(emb, want[1], f"{name} emb")
    for k in want[3]:
        within_grad(grads[k], want[3][k], f"{name} {k}")
    assert_ungathered_rows_are_zero(grads, Pe, X, spec)


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_golden_cases_on_the_device(name):
    """The reference's recorded emb, dense, linear_logit and every recorded gradient through the two modules."""
    fx = R.load_golden(name)
    cols = R.columns_from_fixture(fx)
    fi = build_input_features(cols)
    spec = R.spec_of(cols, fi)
    X = torch.from_numpy(fx["X"])
    lin = linear_module(cols, fi, R.fixture_params(fx, "linear"))
    emb_mod = embedding_module(cols, fi, R.fixture_params(fx, "emb"))
    logit, gl = run_linear(lin, X.to(DEV), torch.from_numpy(fx["c"]))
    emb, dense, ge = run_embedding(emb_mod, X.to(DEV), torch.from_numpy(fx["C"]))
    within_out(logit, torch.from_numpy(fx["out/linear_logit"]), f"{name} linear_logit")
    within_out(emb, torch.from_numpy(fx["out/emb"]), f"{name} emb")
    ns = len(spec.sparse)
    assert torch.equal(emb[:, :ns], torch.from_numpy(fx["out/emb"])[:, :ns])
    assert torch.equal(dense.cpu(), torch.from_numpy(fx["out/dense"]))
    assert sorted(gl) == sorted(R.fixture_params(fx, "grad_linear")) and sorted(ge) == sorted(R.fixture_params(fx, "grad_emb"))
    for k in gl:
        within_grad(gl[k], torch.from_numpy(fx[f"grad_linear/{k}"]), f"{name} linear {k}")
    for k in ge:
        within_grad(ge[k], torch.from_numpy(fx[f"grad_emb/{k}"]), f"{name} emb {k}")


# ---- it plugs in ---------------------------------------------------------------------------------------------------------------
PLUG_B, PLUG_F, PLUG_D, PLUG_DENSE = 260, 19, 16, 3


def plug_columns():
    from satrans_amd.inputs import DenseFeat, SparseFeat
    return [SparseFeat(f"s{i}", 5 + (37 * i) % 90, embedding_dim=PLUG_D) for i in range(PLUG_F)] + [DenseFeat("d", PLUG_DENSE)]


class LibraryModel(nn.Module):
    def __init__(self, cols, fi):
        from satrans_amd import FeatureEmbedding, LinearModel, WDLHead
        super().__init__()
        self.embedding = FeatureEmbedding(cols, fi, init_std=0.1, device=DEV)
        self.linear = LinearModel(cols, fi, init_std=0.1, device=DEV)
        self.head = WDLHead(PLUG_F * PLUG_D + PLUG_DENSE, (32, 16), init_std=0.1).to(DEV)

    def forward(self, X):
        emb, dense = self.embedding(X)
        return torch.sigmoid(self.linear(X) + self.head(torch.cat([emb.flatten(1), dense], dim=1)))


class TorchTwin(nn.Module):
    """The same model with the front end in torch ops (one nn.Embedding call per field, cat, sum, matmul) and the same head;
    the same parameter names, so the library model's state_dict loads as it is.  `reverse`: the order-1 sum in the other order."""

    def __init__(self, cols, fi, reverse=False):
        from satrans_amd import WDLHead
        from satrans_amd.inputs import split_columns
        super().__init__()
        self.sparse, self.dense, _ = split_columns(cols)
        self.fi, self.reverse = fi, reverse
        self.embedding = nn.Module()
        self.embedding.embedding_dict = nn.ModuleDict({c.embedding_name: nn.Embedding(c.vocabulary_size, PLUG_D) for c in self.sparse})
        self.linear = nn.Module()
        self.linear.weight = nn.Parameter(torch.zeros(PLUG_DENSE, 1))
        self.linear.embedding_dict = nn.ModuleDict({c.embedding_name: nn.Embedding(c.vocabulary_size, 1) for c in self.sparse})
        self.head = WDLHead(PLUG_F * PLUG_D + PLUG_DENSE, (32, 16), init_std=0.1)

    def forward(self, X):
        ids = [X[:, self.fi[c.name][0]:self.fi[c.name][1]].long() for c in self.sparse]
        dense = torch.cat([X[:, self.fi[c.name][0]:self.fi[c.name][1]] for c in self.dense], dim=-1)
        emb = torch.cat([self.embedding.embedding_dict[c.embedding_name](i) for c, i in zip(self.sparse, ids)], dim=1)
        first = [self.linear.embedding_dict[c.embedding_name](i) for c, i in zip(self.sparse, ids)]
        if self.reverse:
            first = first[::-1]
        linear_logit = torch.sum(torch.cat(first, dim=-1), dim=-1) + dense.matmul(self.linear.weight)
        return torch.sigmoid(linear_logit + self.head(torch.cat([emb.flatten(1), dense], dim=1)))


def three_adam_steps(model, X, y):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        Fn.binary_cross_entropy(model(X).squeeze(1), y, reduction="sum").backward()
        opt.step()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def test_it_plugs_in_three_adam_steps_against_the_torch_twin():
    """FeatureEmbedding + LinearModel + WDLHead((32, 16)), sigmoid, summed BCE, B = 260, F = 19, D = 16: after three steps of
    torch.optim.Adam(lr = 1e-3) over model.parameters(), every parameter agrees with the torch-ops twin started from the same
    state_dict within 1e-4 max|p| + 5e-9.  The spread of two twin runs that sum the order-1 term in opposite orders is printed
    beside it.  Measured: worst parameter difference 9.3e-4 of the bound, the twin's own spread 5.1e-4 of it - neither comes
    near the bound, which stands as stated."""
    cols = plug_columns()
    fi = build_input_features(cols)
    torch.manual_seed(11)
    model = LibraryModel(cols, fi)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    X = R.draw_X(cols, fi, PLUG_B, g).to(DEV)
    y = (torch.rand(PLUG_B, generator=g) < 0.4).float().to(DEV)
    twins = []
    for reverse in (False, True):
        twin = TorchTwin(cols, fi, reverse).to(DEV)
        twin.load_state_dict(start)
        twins.append(three_adam_steps(twin, X, y))
    got = three_adam_steps(model, X, y)
    assert list(got) == list(twins[0])
    worst = spread = 0.0
    for k, want in twins[0].items():
        bound = GRAD_REL * float(want.abs().max()) + GRAD_ABS
        err = float((got[k] - want).abs().max())
        worst, spread = max(worst, err / bound), max(spread, float((twins[1][k] - want).abs().max()) / bound)
        assert float((want - start[k].cpu()).abs().max()) > 0, k      # the parameter was trained
        assert err <= bound, (k, err, bound)
    print(f"[input] plug-in: worst parameter difference {worst:.2e} of its bound; the twin's own order-of-sum spread {spread:.2e}")
