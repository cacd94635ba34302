"""The descriptor checks of the bf16 evaluation forward (csrc/layer_fwd_bf16.hip) are host code: what they accept and refuse for
the layer variants `gate` / `bilinear`, without a device.  A refused launch returns before it touches the GPU."""
import ctypes as C

import pytest

from satrans_amd import native as N

UNSUPPORTED = -2                                  # SATRANS_E_UNSUPPORTED (include/satrans_hip.h)


def desc(flags, D=32, H=4, U=64, F=19, B=64, S=3, two_tables=False):
    """A descriptor as the checks read it: shape, flags and which pointers are equal (none is dereferenced by a check)."""
    d = N.LayerDesc()
    d.B, d.F, d.D, d.H, d.U, d.S, d.flags = B, F, D, H, U, S, flags
    d.order, d.seg = 0x1000, 0x2000
    d.tab_q, d.tab_k = 0x3000, 0x4000 if two_tables else 0x3000
    d.tab_stride = D * D // H if flags & N.BILINEAR else (D if flags & N.GATE else 2 * D * U)
    return d


def stack_of(d, n=3):
    descs = [d] * n
    return (C.POINTER(N.LayerDesc) * n)(*[C.pointer(x) for x in descs])


@pytest.mark.parametrize("two_tables", [False, True])
@pytest.mark.parametrize("F", [19, 15, 11, 64])
@pytest.mark.parametrize("flags", [N.GATE | N.META_Q | N.META_K, N.GATE | N.META_Q, N.GATE | N.META_K, N.BILINEAR])
def test_gate_and_bilinear_are_built_at_embedding_dim_32(flags, F, two_tables):
    lib = N.lib()
    for U in (64, 32, 7):                         # no MetaNet: its width plays no part
        d = desc(flags, U=U, F=F, two_tables=two_tables)
        assert lib.satrans_layer_fwd_bf16_supported(C.byref(d)) == 1
        assert lib.satrans_stack_fwd_bf16_supported(3, stack_of(d)) == 1
    for extra in (N.RELU_OUT, N.NO_RES):
        assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(flags | extra, F=F))) == 1


@pytest.mark.parametrize("what,d", [
    ("gate and bilinear together", desc(N.GATE | N.BILINEAR | N.META_Q)),
    ("gate in training mode", desc(N.GATE | N.META_Q | N.TRAIN)),
    ("bilinear in training mode", desc(N.BILINEAR | N.TRAIN)),
    ("gate at (D, H) = (64, 4)", desc(N.GATE | N.META_Q, D=64, U=128)),
    ("bilinear at (D, H) = (64, 4)", desc(N.BILINEAR, D=64, U=128)),
    ("gate at (D, H) = (16, 2)", desc(N.GATE | N.META_Q, D=16, H=2, U=32)),
    ("bilinear at (D, H) = (32, 2)", desc(N.BILINEAR, H=2)),
])
def test_what_is_not_built_is_refused_before_any_launch(what, d):
    lib = N.lib()
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(d)) == 0, what
    assert lib.satrans_stack_fwd_bf16_supported(3, stack_of(d)) == 0, what
    y = 0x5000                                    # never written: the refusal comes first
    assert lib.satrans_layer_fwd_bf16(C.byref(d), y, None) == UNSUPPORTED, what
    assert b"gate or bilinear" in lib.satrans_last_error()
    assert lib.satrans_stack_fwd_bf16(3, stack_of(d), y, None) == UNSUPPORTED, what
    assert b"gate or bilinear" in lib.satrans_last_error()
    assert lib.satrans_stack_fwd_bf16_head(3, stack_of(d), C.byref(N.HeadDesc()), None) == UNSUPPORTED, what


def test_the_metanet_form_is_accepted_as_before():
    lib = N.lib()
    meta = N.META_Q | N.META_K
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(meta))) == 1
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(meta, U=32))) == 0            # MetaNet width other than 64
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(0, U=32))) == 1               # no modulation: U plays no part
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(meta, D=64, U=128))) == 1
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(meta, D=64, U=128, F=65))) == 0
    assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(meta | N.TRAIN))) == 0
    assert lib.satrans_stack_fwd_bf16_supported(3, stack_of(desc(meta))) == 1
    assert lib.satrans_stack_fwd_bf16_supported(3, stack_of(desc(meta, D=64, U=128))) == 0  # the stack is built at D = 32
    assert lib.satrans_stack_fwd_bf16_supported(5, stack_of(desc(meta), 5)) == 0
    # a stack whose layers disagree on the variant is no stack
    a, b = desc(N.GATE | N.META_Q), desc(N.BILINEAR)
    arr = (C.POINTER(N.LayerDesc) * 2)(C.pointer(a), C.pointer(b))
    assert lib.satrans_stack_fwd_bf16_supported(2, arr) == 0
