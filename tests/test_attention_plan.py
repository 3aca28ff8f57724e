"""CPU: what cogv_attention_fwd / cogv_attention_bwd decide before they launch (cogv_attention_plan: a host-only query that calls
the function the launches themselves use): the instantiation, grid and dynamic LDS of each kernel, the planes of the sparse
training form, and every refusal with its code.  A wrong LDS size or grid shows on a GPU only as a fault or as idle workgroups.
Every expectation below is a literal worked out by hand from cogview_amd/csrc/attention.hip for the default two-stage ring
(ring 2 x 16384 = 32768 B forward; the backward kernels' rings 32768 / 34816 / 34304 B are raised to the 35840 B of the
column-sum scratch, the dK.dV ring with stored keep bits is 2 x 17984 = 35968 B), not recomputed."""
import ctypes

import pytest

from cogview_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
F16, BF16 = 0, 1
DENSE, DENSE_DROP, DENSE_BITS, FLEXIBLE = 0, 1, 2, 3
PTRS = ("q", "k", "v", "o", "dout", "dq", "dk", "dv", "lse", "dvec")


def desc(B=2, H=40, s_q=1088, s_k=None, **kw):
    """A descriptor whose pointers are dummy non-null, 16-byte aligned integers (never dereferenced by the query)."""
    d = _lib.AttnDesc()
    d.dtype, d.B, d.H, d.s_q, d.s_k, d.head_dim, d.sep = F16, B, H, s_q, s_q if s_k is None else s_k, 64, 0
    d.scale, d.dropout_p, d.seed, d.stream_id = 0.125, 0.0, 1, 2
    for i, name in enumerate(PTRS):
        setattr(d, name, 0x10000 * (i + 1))
    for name in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
        setattr(d, name + "_rs", 3 * H * 64)
        setattr(d, name + "_bs", 3 * H * 64 * max(d.s_q, d.s_k))
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def plan(d, backward):
    """(error code, [form, threads, grid, LDS of forward / dQ, grid, LDS of dK.dV, planes, sep_k])"""
    out = (ctypes.c_int * 8)(*([-1] * 8))
    rc = _lib.lib().cogv_attention_plan(ctypes.byref(d) if d is not None else None, int(backward), out)
    return rc, list(out)


BITS, INDEX, MASK = 0xA0004, 0xB0000, 0xC0002          # 4-byte, 16-byte and 2-byte aligned
SPARSE = dict(B=2, H=3, s_q=640, s_k=296, kv_index=INDEX, sparse_window=128, sparse_pivots=40)      # 40 pivots + 2 x 128 window slots


@pytest.mark.parametrize("kw,backward,want", [
    # the 4B step's shape: 8 x ceil(80 / 8) x 9 = 720 workgroups
    (dict(), 0, [DENSE, 256, 720, 32768, 0, 0, 2, 0]),
    (dict(dropout_p=0.1), 0, [DENSE_DROP, 256, 720, 32768, 0, 0, 2, 0]),
    (dict(dropout_p=0.1, keep_bits=BITS), 0, [DENSE_BITS, 256, 720, 32768, 0, 0, 2, 0]),
    (dict(), 1, [DENSE, 256, 720, 35840, 720, 35840, 2, 0]),
    (dict(dropout_p=0.1), 1, [DENSE_DROP, 256, 720, 35840, 720, 35840, 2, 0]),
    (dict(dropout_p=0.1, keep_bits=BITS), 1, [DENSE_BITS, 256, 720, 35840, 720, 35968, 2, 0]),
    (dict(dtype=BF16, dropout_p=0.1, keep_bits=BITS), 1, [DENSE_BITS, 256, 720, 35840, 720, 35968, 2, 0]),
    # fewer (batch, head) units than XCDs: 8 x 1 x 2
    (dict(B=1, H=3, s_q=192), 0, [DENSE, 256, 16, 32768, 0, 0, 1, 0]),
    (dict(B=1, H=3, s_q=192), 1, [DENSE, 256, 16, 35840, 16, 35840, 1, 0]),
    # sep: the visible prefix in key coordinates, sep + (s_k - s_q)
    (dict(B=1, H=3, s_q=192, sep=5), 0, [DENSE, 256, 16, 32768, 0, 0, 1, 5]),
    (dict(B=1, H=2, s_q=100, s_k=300, sep=5), 0, [DENSE, 256, 8, 32768, 0, 0, 1, 205]),
    (dict(B=1, H=3, s_q=192, sep=-4), 0, [DENSE, 256, 16, 32768, 0, 0, 1, 0]),
    # s_k > s_q: the dK.dV grid follows the keys, 8 x 1 x 3
    (dict(B=1, H=2, s_q=100, s_k=300), 0, [DENSE, 256, 8, 32768, 0, 0, 1, 0]),
    (dict(B=1, H=2, s_q=100, s_k=300), 1, [DENSE, 256, 8, 35840, 24, 35840, 1, 0]),
    # gathered keys, a decode step over 1152 slots: 4608 B of index table behind the ring
    (dict(B=1, H=40, s_q=1, s_k=1152, kv_index=INDEX), 0, [FLEXIBLE, 256, 40, 37376, 0, 0, 1, 0]),
    (dict(B=1, H=40, s_q=1, s_k=1153, kv_index=INDEX), 0, [FLEXIBLE, 256, 40, 37392, 0, 0, 1, 0]),      # 4612 -> 4624
    (dict(B=1, H=40, s_q=1, s_k=4096, kv_index=INDEX, dropout_p=0.1, keep_bits=BITS), 0, [FLEXIBLE, 256, 40, 49152, 0, 0, 1, 0]),
    # sparse training form: 296 slots = 1184 B of table; backward 2 x 5 planes -> 8 x ceil(30 / 8) x 3 workgroups
    (SPARSE, 0, [FLEXIBLE, 256, 40, 33952, 0, 0, 2, 0]),
    (SPARSE, 1, [FLEXIBLE, 256, 40, 37024, 96, 35840, 10, 0]),
    (dict(SPARSE, dropout_p=0.1, keep_bits=BITS), 1, [FLEXIBLE, 256, 40, 37024, 96, 35840, 10, 0]),   # keep bits: dense form only
    # a mask tensor: the flexible instantiation, every key a candidate
    (dict(B=2, H=3, s_q=192, mask=MASK), 0, [FLEXIBLE, 256, 16, 32768, 0, 0, 2, 192]),
    (dict(B=2, H=3, s_q=192, mask=MASK, sep=7, dropout_p=0.1), 1, [FLEXIBLE, 256, 16, 35840, 16, 35840, 2, 192]),
    (dict(B=2, H=3, s_q=100, s_k=300, mask=MASK), 1, [FLEXIBLE, 256, 8, 35840, 24, 35840, 2, 300]),
    # the fused bias gradient changes nothing about the launches
    (dict(colsum_partial=0xD0000), 1, [DENSE, 256, 720, 35840, 720, 35840, 2, 0]),
])
def test_plan(kw, backward, want):
    assert plan(desc(**kw), backward) == (OK, want)


def test_plan_dropout_below_the_16_bit_threshold_is_no_dropout():
    """thr16 = (uint32_t)(p * 65536 + 0.5): p < 2^-17 leaves it 0; stored bits are then ignored (even a misaligned pointer)."""
    for backward, lds in ((0, [720, 32768, 0, 0]), (1, [720, 35840, 720, 35840])):
        assert plan(desc(dropout_p=7e-6), backward) == (OK, [DENSE, 256] + lds + [2, 0])
        assert plan(desc(dropout_p=7e-6, keep_bits=BITS), backward) == (OK, [DENSE, 256] + lds + [2, 0])
        assert plan(desc(dropout_p=7e-6, keep_bits=BITS + 1), backward) == (OK, [DENSE, 256] + lds + [2, 0])
        assert plan(desc(dropout_p=8e-6), backward) == (OK, [DENSE_DROP, 256] + lds + [2, 0])
    assert plan(desc(dropout_p=8e-6, keep_bits=BITS), 0) == (OK, [DENSE_BITS, 256, 720, 32768, 0, 0, 2, 0])
    assert plan(desc(dropout_p=8e-6, keep_bits=BITS), 1) == (OK, [DENSE_BITS, 256, 720, 35840, 720, 35968, 2, 0])


BOTH = [
    (dict(dtype=2), ERR_UNSUPPORTED), (dict(dtype=-1), ERR_UNSUPPORTED), (dict(head_dim=128), ERR_UNSUPPORTED),
    (dict(B=0), ERR_ARG), (dict(H=0), ERR_ARG), (dict(s_q=0, s_k=64), ERR_ARG), (dict(s_k=-1), ERR_ARG), (dict(B=-2), ERR_ARG),
    (dict(s_q=192, s_k=128), ERR_ARG),                                              # s_k < s_q outside slot space
    (dict(s_q=192, s_k=128, sparse_window=128), ERR_ARG),
    (dict(dropout_p=1.0), ERR_ARG), (dict(dropout_p=-0.1), ERR_ARG), (dict(dropout_p=float("nan")), ERR_ARG),
    (dict(mask=MASK, kv_index=INDEX), ERR_ARG), (dict(mask=MASK, keep_bits=BITS), ERR_ARG), (dict(mask=MASK + 1), ERR_ARG),
    (dict(SPARSE, s_k=4224, sparse_pivots=40), ERR_UNSUPPORTED),                    # more than 4096 slots
    (dict(SPARSE, sparse_window=64), ERR_ARG), (dict(SPARSE, sparse_window=192, s_q=576), ERR_ARG),     # not a multiple of 128
    (dict(SPARSE, s_q=704), ERR_ARG),                                               # s_q not a multiple of the window
    (dict(SPARSE, sparse_pivots=-1), ERR_ARG), (dict(SPARSE, sparse_pivots=297), ERR_ARG),
    (dict(SPARSE, sparse_window=384, s_q=768), ERR_ARG),                            # fewer slots than the window
    (dict(SPARSE, sep=3), ERR_ARG),
    (dict(sparse_window=128), ERR_ARG),                                             # a sparse window without an index
    (dict(q=0), ERR_ARG), (dict(o=0), ERR_ARG),
    (dict(q=0x10008), ERR_ARG), (dict(k=0x20004), ERR_ARG), (dict(v=0x30002), ERR_ARG), (dict(o=0x40001), ERR_ARG),
    (dict(q_rs=7684), ERR_ARG), (dict(o_rs=7), ERR_ARG), (dict(k_bs=12), ERR_ARG), (dict(v_bs=-4), ERR_ARG),
    (dict(dropout_p=0.1, keep_bits=BITS + 2), ERR_ARG), (dict(dropout_p=0.1, keep_bits=BITS + 1), ERR_ARG),
]
FORWARD_ONLY = [
    (dict(B=1, s_q=1, s_k=4097, kv_index=INDEX), ERR_UNSUPPORTED),
    (dict(B=1, s_q=1, s_k=4097, kv_index=INDEX, q=0x10008), ERR_ARG),               # forward: alignment before the index
]
BACKWARD_ONLY = [
    (dict(B=1, s_q=1, s_k=1152, kv_index=INDEX), ERR_UNSUPPORTED),                  # the plain gathered form is inference only
    (dict(B=1, s_q=1, s_k=1152, kv_index=INDEX, q=0x10008), ERR_UNSUPPORTED),       # backward: the index before alignment
    (dict(SPARSE, colsum_partial=0xD0000), ERR_UNSUPPORTED),
    (dict(s_q=192, s_k=320, colsum_partial=0xD0000), ERR_ARG), (dict(colsum_partial=0xD0008), ERR_ARG),
    (dict(dout=0), ERR_ARG), (dict(dq=0), ERR_ARG), (dict(dk=0), ERR_ARG), (dict(dv=0), ERR_ARG), (dict(lse=0), ERR_ARG), (dict(dvec=0), ERR_ARG),
    (dict(dout=0x50008), ERR_ARG), (dict(dq=0x60004), ERR_ARG), (dict(dk=0x70002), ERR_ARG), (dict(dv=0x80001), ERR_ARG),
    (dict(do_rs=4), ERR_ARG), (dict(dq_rs=-2), ERR_ARG), (dict(dk_bs=4), ERR_ARG), (dict(dv_bs=9), ERR_ARG),
]


@pytest.mark.parametrize("kw,rc,backward", [(kw, rc, b) for kw, rc in BOTH for b in (0, 1)] + [(kw, rc, 0) for kw, rc in FORWARD_ONLY] +
                         [(kw, rc, 1) for kw, rc in BACKWARD_ONLY])
def test_plan_refuses_what_the_launch_refuses(kw, rc, backward):
    """... with the launch's code, and leaves `out` untouched."""
    assert plan(desc(**kw), backward) == (rc, [-1] * 8)


def test_backward_only_fields_do_not_disturb_forward():
    """What only the backward call reads (gradient pointers and strides, the column-sum workspace) is not checked by the forward call."""
    for kw, _ in BACKWARD_ONLY[3:]:
        assert plan(desc(**kw), 0)[0] == OK, kw
    assert plan(None, 0)[0] == ERR_ARG and plan(None, 1)[0] == ERR_ARG
