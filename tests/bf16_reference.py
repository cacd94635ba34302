"""Rounding model of the bf16 evaluation forward (satrans_amd/csrc/layer_fwd_bf16.hip)  --  TEST INFRASTRUCTURE.

The kernels round at known points only: `stage_bf16` / `stage_bilinear` round every weight image, `chain_bf16` rounds the fp32
fragment that enters each product.  Everything else is fp32.  This module restates `layer_forward` / `metanet` of
oracle/satrans_oracle.py with exactly those roundings in, over the same state_dict-shaped dict, in fp64 or in fp32 (the dtype
of the dict and of the input decides).  What is left between the model and a kernel is the accumulation order and a rare bf16
"flip": an intermediate that falls on the other side of a rounding boundary in another evaluation order.

  rounded weights      W_Query, W_Key, W_Value, Out_linear.weight, the generated W1 / W2 of each modulated role, the H generated
                       d x d maps of 'bilinear'
  rounded activations  x into the three projections, q0 / k0 into W1, relu(h) into W2, the attention output into Out_linear,
                       q into the bilinear maps
  not rounded          residuals, both LayerNorms (eps 1e-6), scores, softmax, P V, the gate's multiplication by 2 vec, relu on the
                       output, the head (flatten + dense columns + dnn_linear)

`Rounding` switches the points off one by one; all off is the oracle.  `criterion` / `check_*` are the ONE comparison the CPU
and the GPU tests share, `tile_*` restate the launchers' tile choosers, and `CASES` is the list of shapes both test modules walk.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import satrans_oracle as O

Tensor = torch.Tensor


def rbf16(t: Tensor) -> Tensor:
    """Round to nearest even onto the bf16 grid, through torch.bfloat16 and back to t.dtype.

    From fp64 torch converts by way of fp32, and a value that the first rounding puts exactly on a bf16 tie would then go to the
    even neighbour whichever side of the tie it came from.  Such a value is moved one fp32 step back towards where it was
    before the second rounding (round-to-odd on the way, in effect), which makes the result the single RNE rounding."""
    if t.dtype == torch.float64:
        f = t.float()
        d = t - f.double()
        tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
        fix = tie & (d != 0) & torch.isfinite(f)
        if bool(fix.any()):
            toward = torch.where(d > 0, torch.full_like(f, math.inf), torch.full_like(f, -math.inf))
            f = torch.where(fix, torch.nextafter(f, toward), f)
        return f.bfloat16().double()
    return t.bfloat16().to(t.dtype)


@dataclass(frozen=True)
class Rounding:
    """The kernels' rounding points.  ALL_OFF turns the model into the oracle."""
    weights: bool = True        # W_Query / W_Key / W_Value / Out_linear images (stage_bf16)
    generated: bool = True      # generated W1 / W2 images (stage_bf16), bilinear maps (stage_bilinear)
    x: bool = True              # x into the three projections
    meta_in: bool = True        # q0 / k0 into W1
    hidden: bool = True         # relu(h) into W2
    attn_out: bool = True       # attention output into Out_linear
    bilinear_q: bool = True     # q into the bilinear maps


ALL_ON = Rounding()
ALL_OFF = Rounding(False, False, False, False, False, False, False)

# Deliberate faults of the MODEL (tests/test_bf16_reference_cpu.py: the criterion must tell each from the unmutated model)
FAULT_W2_SWAP = "w2_swap"               # two contraction indices of W2 swapped within the last K-step of 32
FAULT_K_LN_FROM_Q = "k_ln_from_q"       # the K-side MetaNet LayerNorm reads the Q-side vectors
FAULT_PAD_KEYS = "pad_keys"             # the padded keys of the last chunk of four are counted into the softmax sum


def _r(on: bool, t: Tensor) -> Tensor:
    return rbf16(t) if on else t


def metanet(z: Tensor, vec: Tensor, gamma: Tensor, beta: Tensor, spec: O.PathSpec, R: Rounding, fault: str = "") -> Tensor:
    """O.metanet (two matrices, evaluation) with the rounding in: LN(relu(r(z) r(W1)) r(W2) + z)."""
    D, U = spec.meta_units[0], spec.meta_units[1]
    W1 = _r(R.generated, vec[:, :D * U].reshape(-1, D, U))
    W2 = _r(R.generated, vec[:, D * U:D * U + U * D].reshape(-1, U, D))
    if fault == FAULT_W2_SWAP:
        idx = torch.arange(U)
        idx[U - 32 + 5], idx[U - 32 + 22] = U - 32 + 22, U - 32 + 5
        W2 = W2[:, idx, :]
    h = torch.relu(torch.matmul(_r(R.meta_in, z), W1))
    o = torch.matmul(_r(R.hidden, h), W2)
    return F.layer_norm(o + z, (D,), gamma, beta, 1e-6)


def layer(P: Dict[str, Tensor], l: int, x: Tensor, vecs: List[Tensor], spec: O.PathSpec, R: Rounding = ALL_ON,
          fault: str = "") -> Tensor:
    """One Meta_Transformer_Layer (evaluation) applied to x [B, F, D]: O.layer_forward with the kernels' rounding points."""
    pre = f"domain_int_layers.{l}."
    D, H = spec.embedding_dim, spec.head_num
    d = D // H
    xr = _r(R.x, x)
    q = xr @ _r(R.weights, P[pre + "W_Query"])
    k = xr @ _r(R.weights, P[pre + "W_Key"])
    v = xr @ _r(R.weights, P[pre + "W_Value"])
    gate, bilinear = "gate" in spec.flag, "bilinear" in spec.flag
    if "Q" in spec.meta_mode and not bilinear:
        if gate:
            q = q * vecs[0].unsqueeze(1) * 2
        else:
            q = metanet(q, vecs[0], P[pre + "Q_meta_mlp.ffn_layer_norm.weight"], P[pre + "Q_meta_mlp.ffn_layer_norm.bias"],
                        spec, R, fault)
    if "K" in spec.meta_mode and not bilinear:
        if gate:
            k = k * vecs[1].unsqueeze(1) * 2
        else:
            side = "Q" if fault == FAULT_K_LN_FROM_Q else "K"
            k = metanet(k, vecs[1], P[pre + f"{side}_meta_mlp.ffn_layer_norm.weight"],
                        P[pre + f"{side}_meta_mlp.ffn_layer_norm.bias"], spec, R, fault)
    B, Fn, _ = x.shape
    qh = q.reshape(B, Fn, H, d).permute(0, 2, 1, 3)
    kh = k.reshape(B, Fn, H, d).permute(0, 2, 1, 3)
    vh = v.reshape(B, Fn, H, d).permute(0, 2, 1, 3)
    if bilinear:
        M = _r(R.generated, vecs[0][:, :H * d * d].reshape(-1, H, d, d))
        qh = _r(R.bilinear_q, qh) @ M
    s = qh @ kh.transpose(-1, -2) / (d ** 0.5)
    if fault == FAULT_PAD_KEYS and Fn % 4:
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        a = e / (e.sum(-1, keepdim=True) + (4 - Fn % 4) * e[..., -1:])       # (the padding reads the last real key's row)
    else:
        a = torch.softmax(s, dim=-1)
    o = (a @ vh).permute(0, 2, 1, 3).reshape(B, Fn, D)
    o = _r(R.attn_out, o) @ _r(R.weights, P[pre + "Out_linear.weight"]).t()
    if "relu" in spec.flag:
        o = torch.relu(o)
    if spec.use_res:
        o = o + x
    return F.layer_norm(o, (D,), P[pre + "layer_norm.weight"], P[pre + "layer_norm.bias"], 1e-6)


def head(P: Dict[str, Tensor], y: Tensor, X: Tensor, spec: O.PathSpec) -> Tensor:
    """Logits [B] behind the last layer's output y: flatten + dense columns + dnn_linear, nothing rounded."""
    flat = y.flatten(1)
    dense = O.dense_block(X, spec)
    if dense is not None:
        flat = torch.cat([flat, dense.to(flat.dtype)], dim=-1)
    return F.linear(flat, P["dnn_linear.weight"], P["dnn_linear.bias"]).reshape(-1)


def forward(P: Dict[str, Tensor], X: Tensor, spec: O.PathSpec, R: Rounding = ALL_ON, fault: str = "") -> Tuple[List[Tensor], Tensor]:
    """-> ([gathered rows, layer 0 output, ...], logits [B]) of a compounded forward."""
    x = O.gather_fields(P, X, spec)
    vecs = O.scenario_vectors(P, X, spec)
    outs = [x]
    for l in range(spec.layer_num):
        outs.append(layer(P, l, outs[-1], vecs[l], spec, R, fault))
    return outs, head(P, outs[-1], X, spec)


def as_double(P: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The dict in fp64, aliased keys still one tensor."""
    conv: Dict[int, Tensor] = {}
    return {k: conv.setdefault(id(v), v.double()) for k, v in P.items()}


class Triple:
    """The three references of one case: the model in fp64 and in fp32 and the exact fp64 oracle, each applied to a GIVEN layer
    input so that the errors of the layers do not compound - and to GIVEN generated rows.  `vecs` (per layer [vec_Q, vec_K],
    fp32 [B, P]): the rows the kernels read, i.e. the engine's scenario table indexed by the samples' scenario; default: the
    oracle's own in fp32.  All three use the same fp32 values: a generated weight that the fp32 and the fp64 encoder put on
    different sides of a bf16 boundary would move one output feature of EVERY token of a scenario, and the encoder is another
    kernel's business (tests/test_scenario_kernels_gpu.py)."""

    def __init__(self, P32: Dict[str, Tensor], X: Tensor, spec: O.PathSpec, vecs: Optional[List[List[Tensor]]] = None):
        self.P32, self.P64, self.X, self.spec = P32, as_double(P32), X, spec
        self.v32 = vecs if vecs is not None else O.scenario_vectors(P32, X, spec)
        self.v64 = [[v.double() for v in trio] for trio in self.v32]

    def layer(self, l: int, x: Tensor, fault: str = "", R: Rounding = ALL_ON):
        """x: fp32 [B, F, D]  ->  (m64, m32, ex)"""
        x32, x64 = x.float(), x.double()
        return (layer(self.P64, l, x64, self.v64[l], self.spec, R, fault), layer(self.P32, l, x32, self.v32[l], self.spec, R, fault),
                layer(self.P64, l, x64, self.v64[l], self.spec, ALL_OFF))

    def logits(self, y_last: Tensor, ex_last: Tensor):
        """y_last: the last layer's output as computed (fp32); ex_last: the exact oracle's output of that layer for the same
        layer input  ->  (m64, m32, ex).  The head rounds nothing, so the rounding effect on the logits is the last layer's."""
        return (head(self.P64, y_last.double(), self.X, self.spec), head(self.P32, y_last.float(), self.X, self.spec),
                head(self.P64, ex_last.double(), self.X, self.spec))


# --------------------------------------------------------------------------------------------------------------------------
# The comparison criterion
# --------------------------------------------------------------------------------------------------------------------------
TIGHT_SHARE = 5e-3          # at most this share of the elements of `got` further than T from m64
M32_SHARE = 2e-3            # ... and of the model in fp32 (a condition on the reference alone)
RESOLUTION = 5e-2           # at least this share of the exact oracle's elements further than T from m64


def criterion(got: Optional[Tensor], m64: Tensor, m32: Tensor, ex: Tensor) -> Dict[str, float]:
    """T = max(8 q99(|m32 - m64|), 2e-6 max|m64|): the CPU's two summation orders differ by q99 at the 99th percentile (the
    maximum is set by flips); the kernel's order is a third one, hence the factor 8.  E = max|m64 - ex|: the largest effect of
    the rounding on this tensor; one flipped operand moves a product by less than the rounding of all operands together."""
    m64 = m64.double()
    dm = (m32.double() - m64).abs().reshape(-1)
    de = (ex.double() - m64).abs().reshape(-1)
    T = max(8.0 * float(torch.quantile(dm, 0.99)), 2e-6 * float(m64.abs().max()))
    E = float(de.max())
    out = {"T": T, "E": E, "m32_share": float((dm > T).double().mean()), "m32_loose": float(dm.max()) / max(E, 1e-300),
           "resolution": float((de > T).double().mean())}
    if got is not None:
        err = (got.double() - m64).abs().reshape(-1)
        inside = err[err <= T]
        out.update(share=float((err > T).double().mean()), tight=float(inside.max()) / T if inside.numel() else 0.0,
                   loose=float(err.max()) / max(E, 1e-300), err=float(err.max()))
    return out


def check_reference(c: Dict[str, float], msg, resolution: bool = True, m32: bool = True) -> None:
    """The conditions on the reference alone: without them a case cannot hold a kernel to anything.  (m32 = False: the GPU test,
    where the layer inputs are the kernel's and the fp32 model's share is a figure to print; the CPU test asserts it.)"""
    if m32:
        assert c["m32_share"] <= M32_SHARE, (msg, "the model in fp32 leaves the tight tier", c)
    assert c["m32_loose"] <= 1.0, (msg, "the model in fp32 leaves the loose tier", c)
    if resolution:
        assert c["resolution"] >= RESOLUTION, (msg, "the case cannot tell a bf16 kernel from an fp32 one", c)


def check_got(c: Dict[str, float], msg, tight: bool = True) -> None:
    if tight:
        assert c["share"] <= TIGHT_SHARE, (msg, "tight tier", c)
    assert c["loose"] <= 1.0, (msg, "loose tier", c)


def fails(c: Dict[str, float], tight: bool = True) -> bool:
    return (tight and c["share"] > TIGHT_SHARE) or c["loose"] > 1.0


# --------------------------------------------------------------------------------------------------------------------------
# The launchers' tile choosers, restated (launch_fwd_bf16 / launch_stack_bf16)
# --------------------------------------------------------------------------------------------------------------------------
def _image_elems(D, U, same_tab, mod):
    KD, KU = D + 8, U + 8
    if mod:
        return (5 if mod == 2 else 4) * D * KD
    return 4 * D * KD + (1 if same_tab else 2) * (U * KD + D * KU)


def _vectors(mod):
    return {0: 6, 1: 4, 2: 2}[mod]


def lds_bytes(T, F_, D, U, same_tab, mod, stack_layers=0):
    rows = (T * F_ + 15) // 16 * 16
    if stack_layers:
        return 2 * _image_elems(D, U, same_tab, mod) * stack_layers + 4 * (_vectors(mod) * D * stack_layers + 4 * rows * (D + 4)) + 256
    return 2 * _image_elems(D, U, same_tab, mod) + 4 * (_vectors(mod) * D + 3 * rows * (D + 4)) + 256


def tile_samples(F_, D, same_tab, mod, stack_layers=0) -> int:
    """Samples per tile of the layer launch (stack_layers = 0) or of the stacked launch; 0: does not fit LDS."""
    U, H, waves = (64, 4, 12) if D == 32 else (128, 4, 8)
    ft = F_ if (D == 32 and F_ in (15, 19)) else 0
    limit = 160 * 1024 if stack_layers else 156 * 1024
    best, best_eff = 0, 0.0
    for t in range(1, 4 * waves + 1):
        if lds_bytes(t, F_, D, U, same_tab, mod, stack_layers) > limit:
            break
        tok = t * F_
        ntt = (tok + 15) // 16
        eff = tok / (16.0 * ntt) * ntt / (-(-ntt // waves) * waves)
        if ft:
            per_round, groups = waves * (64 // ((ft + 3) & ~3)), t * H
            eff_att = groups / (-(-groups // per_round) * per_round)
            eff = 1.0 / (0.5 / eff + 0.5 / eff_att) if stack_layers else 1.0 / (0.35 / eff + 0.65 / eff_att)
        if eff >= best_eff:
            best_eff, best = eff, t
    return best


# --------------------------------------------------------------------------------------------------------------------------
# The cases both test modules walk
# --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    """A synthetic model (helpers.SyntheticModel) and its batch.  `stack`: the one-launch stack serves it (expected answer of
    satrans_stack_fwd_bf16_supported).  `supported`: expected answer of satrans_layer_fwd_bf16_supported.  `emb` / `gen`:
    factors on the embedding tables / the scenario encoder's weight.  `tight`: False keeps the case on the loose tier only."""
    name: str
    D: int
    H: int
    U: int
    F: int
    flag: str = "sota"
    mode: str = "QK"
    L: int = 2
    B: int = 0                  # 0: 400 (scenario_ids says why)
    n_dense: int = 0
    stack: bool = True
    supported: bool = True
    emb: float = 300.0
    gen: float = 1.0
    tight: bool = True
    # Vocabulary sizes of the fields are drawn from this range: above the batch size, so that a layer-0 token (an embedding row)
    # seldom repeats.  The criterion's shares take flips for independent events.  With the 5 - 60 ids per field of the other
    # synthetic models a row sits in 10 - 100 of 400 samples and ONE flip counts that many times: at F = 37 with 'pos' one
    # element of k0 = r(x) r(W_Key) of one row of field 7 lies 3.8e-6 of a bf16 step from a tie (sums of 32 products of bf16
    # numbers land near ties far more often than reals do), the kernel's order rounds it the other way than fp64 does, and
    # every sample that holds that row moves by ~4e-6 in all its tokens - 4 % of the layer at B = 50, 1.5 % at B = 400, where
    # putting that one operand on the other side in the model brings the kernel's output of those samples back within 6e-7.
    vocab: Tuple[int, int] = (600, 1200)

    @property
    def mod(self) -> int:
        return 1 if "gate" in self.flag else (2 if "bilinear" in self.flag else 0)

    @property
    def same_tab(self) -> bool:
        return "pos" not in self.flag

    def tiles(self) -> Tuple[int, int]:
        """(samples per tile of the layer launch, ... of the stacked launch or 0)"""
        if not self.supported:
            return 0, 0
        return (tile_samples(self.F, self.D, self.same_tab, self.mod),
                tile_samples(self.F, self.D, self.same_tab, self.mod, self.L) if self.stack else 0)

    def scenario_ids(self):
        """[B] ids in 1..3 (id 0 stays empty): scenario 1 holds a full tile followed by a partial one of BOTH launches, 2 and 3
        hold what is left.  B as given, else 400.  Why not 21 or 50: between two evaluation orders about one token in 300 has an
        operand on the other side of a bf16 boundary (a "flip"; measured on the CPU, fp32 against fp64 model, B = 600).  A flip on
        the query side or behind the attention moves the D outputs of its token; one on the key side moves every token of its
        SAMPLE, by about 1 / F of the flip, which is about T.  The criterion's shares (2e-3, 5e-3) count elements, so they mean
        something only where one sample is well under them: at B = 50 one sample is 2 % of the tensor, at B = 400 it is 0.25 %."""
        import numpy as np
        Tl, Ts = self.tiles()
        Ts = Ts or Tl

        def first(B):
            for n1 in range(max(Tl, Ts) + 1, B - 1):
                if (Tl == 1 or n1 % Tl) and (Ts == 1 or n1 % Ts):
                    return n1
            return 0

        if not self.supported:
            B, n1 = self.B or 21, 12
        elif self.B:
            B, n1 = self.B, first(self.B) or max(1, self.B - 2)
        else:
            B = 400
            n1 = first(B)
        rest = B - n1
        ids = np.array([1] * n1 + [2] * (rest - rest // 2) + [3] * (rest // 2), dtype=np.int64)
        return np.random.RandomState(B + self.F).permutation(ids)

    @property
    def seed(self) -> int:
        return SEEDS.get(self.name, 0)


# Seed of a case's id matrix where it is not 0: the first for which the model ALONE meets the criterion's conditions on a
# reference (fp32 model within 2e-3 of the tight tier at every layer; tests/test_bf16_reference_cpu.py asserts them).  Found on the
# CPU from the model in fp32 and fp64, before any kernel ran.
SEEDS: Dict[str, int] = {"d32-F15-QK": 2, "d32-F37-pos": 7, "d64-F5": 43, "d64-F13-Q": 1, "d32-F15-L1": 1, "d32-F15-L5": 15,
                         "d32-F19-B3000": 8}

_D32 = dict(D=32, H=4, U=64)
_D64 = dict(D=64, H=4, U=128, stack=False)          # the stack is built at D = 32

CASES: List[Shape] = (
    # constant-F arm (the 4x4 MFMA attention), every meta_mode: same_tab staging with one or both roles, nothing modulated
    [Shape(f"d32-F{F_}-{m or 'none'}", **_D32, F=F_, mode=m) for F_ in (19, 15) for m in ("QK", "Q", "K", "")] + [
    Shape("d32-F19-pos", **_D32, F=19, flag="sota-pos"),             # two tables: w1k / w2k carved separately
    Shape("d32-F19-pos-K", **_D32, F=19, flag="sota-pos", mode="K"),
    Shape("d32-F19-relu", **_D32, F=19, flag="sota-relu"),           # SATRANS_RELU_OUT
    # run-time arm: F % 4 = 3, 1, 2, 0, and F > 32
    Shape("d32-F11", **_D32, F=11), Shape("d32-F5-K", **_D32, F=5, mode="K"), Shape("d32-F6-Q", **_D32, F=6, mode="Q"),
    Shape("d32-F8", **_D32, F=8), Shape("d32-F33", **_D32, F=33), Shape("d32-F37-pos", **_D32, F=37, flag="sota-pos"),
    Shape("d32-F11-none-U48", D=32, H=4, U=48, F=11, mode=""),       # nothing modulated: any U
    # (D, U, H) = (64, 128, 4) on 8 waves: four K-steps into W2
    Shape("d64-F5", **_D64, F=5), Shape("d64-F13", **_D64, F=13), Shape("d64-F13-Q", **_D64, F=13, mode="Q"),
    Shape("d64-F33-Q", **_D64, F=33, mode="Q"), Shape("d64-F33", **_D64, F=33), Shape("d64-F64", **_D64, F=64),
    Shape("d64-F13-pos", **_D64, F=13, flag="sota-pos"),
    # gate and bilinear (the maps are a rounding point of their own)
    Shape("d32-F19-gate", **_D32, F=19, flag="sota-gate"), Shape("d32-F11-gate", **_D32, F=11, flag="sota-gate"),
    Shape("d32-F19-bilinear", **_D32, F=19, flag="sota-bilinear"), Shape("d32-F11-bilinear", **_D32, F=11, flag="sota-bilinear"),
    # stack depth (L = 2 at F = 15 is d32-F15-QK): 1, 3, 4 in one launch; 5 is refused by the stack query -> layer launches.
    # (3 and 4 layers modulate one side only: with both, the fp32 model's share outside T sits AT its bound of 2e-3 at F = 15 -
    #  0.17 - 0.22 % per layer at B = 400 - and no id matrix in 80 kept three layers in a row under it)
    Shape("d32-F15-L1", **_D32, F=15, L=1), Shape("d32-F15-L3-Q", **_D32, F=15, L=3, mode="Q"), Shape("d32-F15-L4-K", **_D32, F=15, L=4, mode="K"),
    Shape("d32-F15-L5", D=32, H=4, U=64, F=15, L=5, stack=False),
    # dense columns behind the stacked head
    Shape("d32-F19-dense1", **_D32, F=19, n_dense=1), Shape("d32-F19-dense2", **_D32, F=19, n_dense=2),
    # one sample; more tiles than workgroups (B = 3000)
    Shape("d32-F19-B1", **_D32, F=19, B=1), Shape("d32-F19-B3000", **_D32, F=19, B=3000),
])

# what the bf16 entry points refuse: the forward under "bf16" is then the fp32 kernels' bits
REFUSED: List[Shape] = [
    Shape("d64-F65", D=64, H=4, U=128, F=65, stack=False, supported=False),
    Shape("d64-F49-pos", D=64, H=4, U=128, F=49, flag="sota-pos", stack=False, supported=False),   # two tables: does not fit LDS
    Shape("d32-H8", D=32, H=8, U=64, F=11, stack=False, supported=False),
]

GOLDEN = ["aliccp_sota", "alimama_sota_pos"]


def full_then_partial(ids, T: int) -> bool:
    """Some scenario holds a full tile of T samples followed by a partial one (T = 1: more than one tile)."""
    import numpy as np
    return any(c > T and (T == 1 or c % T) for c in np.bincount(np.asarray(ids, dtype=np.int64)))


def case_by_name(name: str) -> Shape:
    return next(c for c in CASES + REFUSED if c.name == name)
