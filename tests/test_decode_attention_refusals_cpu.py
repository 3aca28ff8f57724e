"""CPU: the return code of each decode-attention entry point for a descriptor with ONE broken field.

cogv_attention_decode, cogv_attention_decode_chunk and cogv_attention_decode_kv8 share one host path; what each returns for a
single fault is part of the C ABI (include/cogview_hip.h) and differs between them in two places (a NULL descriptor, head_dim
!= 64).  The descriptors are built from fake, suitably aligned, non-zero addresses and every call made here is refused: nothing
is launched and no pointer is dereferenced.  The precedence between two simultaneous faults is not part of the contract.
"""
import ctypes as C

import pytest

from cogview_amd import _lib

F16, F32 = 0, 2
B, H, CAP, M = 2, 3, 384, 4
HP = H * 64
ENTRIES = ("decode", "chunk", "kv8")


def _valid(entry):
    """A descriptor the entry point would accept (never passed on as it is)."""
    lib = _lib.lib()
    rows = B * M if entry == "chunk" else B
    ws_bytes = lib.cogv_attention_decode_workspace_bytes(rows, H, CAP)
    assert ws_bytes == rows * H * 3 * 66 * 4
    d = {"decode": _lib.AttnDecodeDesc, "chunk": _lib.AttnDecodeChunkDesc, "kv8": _lib.AttnDecodeKv8Desc}[entry]()
    d.dtype, d.B, d.H, d.capacity, d.head_dim, d.scale = F16, B, H, CAP, 64, 0.125
    d.qkv, d.out, d.pos, d.workspace, d.first = 0x100000, 0x300000, 0x400000, 0x500000, 0x600000
    d.workspace_bytes, d.skip_combine = ws_bytes, 0
    if entry == "chunk":
        d.m, d.qkv_rs, d.out_rs = M, 3 * HP, HP
    else:
        d.qkv_bs, d.out_bs = 3 * HP, HP
    if entry == "kv8":
        d.kv_q, d.kv_q_bs, d.kv_scale, d.kv_scale_bs = 0x700000, 2 * H * CAP * 64, 0x800000, 2 * H * CAP
    else:
        d.cache, d.cache_bs, d.cache_rs = 0x200000, CAP * 2 * HP, 2 * HP
    return d


def _call(entry, d):
    fn = getattr(_lib.lib(), {"decode": "cogv_attention_decode", "chunk": "cogv_attention_decode_chunk", "kv8": "cogv_attention_decode_kv8"}[entry])
    return fn(C.byref(d) if d is not None else None, None)


ROOMY = 1 << 40        # workspace_bytes that no shape of this file exceeds: the fault under test stays the only one
QKV_STRIDE = {"decode": "qkv_bs", "chunk": "qkv_rs", "kv8": "qkv_bs"}

# fault, the fields it sets ("qkv_stride": qkv_bs or qkv_rs), and the code of (decode, chunk, kv8); None: the entry point has no
# such field.  1: bad argument, 3: unsupported.  Recorded from the library before the three host paths became one.
FAULTS = [
    ("qkv NULL", {"qkv": None}, (1, 1, 1)),
    ("cache NULL", {"cache": None}, (1, 1, None)),
    ("kv_q NULL", {"kv_q": None}, (None, None, 1)),
    ("kv_scale NULL", {"kv_scale": None}, (None, None, 1)),
    ("pos NULL", {"pos": None}, (1, 1, 1)),
    ("workspace NULL", {"workspace": None}, (1, 1, 1)),
    ("out NULL without skip_combine", {"out": None}, (1, 1, 1)),
    ("qkv not 16-byte aligned", {"qkv": 0x100008}, (1, 1, 1)),
    ("cache not 16-byte aligned", {"cache": 0x200008}, (1, 1, None)),
    ("kv_q not 16-byte aligned", {"kv_q": 0x700008}, (None, None, 1)),
    ("kv_scale not 4-byte aligned", {"kv_scale": 0x800002}, (None, None, 1)),
    ("first not 4-byte aligned", {"first": 0x600002}, (1, 1, 1)),
    ("workspace not 16-byte aligned", {"workspace": 0x500008}, (1, 1, 1)),
    ("qkv stride % 8", {"qkv_stride": 3 * HP + 4}, (1, 1, 1)),
    ("cache_bs % 8", {"cache_bs": CAP * 2 * HP + 4}, (1, 1, None)),
    ("cache_rs % 8", {"cache_rs": 2 * HP + 4}, (1, 1, None)),
    ("kv_q_bs % 16", {"kv_q_bs": 2 * H * CAP * 64 + 8}, (None, None, 1)),
    ("kv_q_bs short", {"kv_q_bs": 2 * H * CAP * 64 - 16}, (None, None, 1)),
    ("kv_scale_bs short", {"kv_scale_bs": 2 * H * CAP - 1}, (None, None, 1)),
    ("B = 0", {"B": 0}, (1, 1, 1)),
    ("B = -1", {"B": -1}, (1, 1, 1)),
    ("H = 0", {"H": 0}, (1, 1, 1)),
    ("H = -1", {"H": -1}, (1, 1, 1)),
    ("capacity = 0", {"capacity": 0}, (1, 1, 1)),
    ("capacity = -128", {"capacity": -128}, (1, 1, 1)),
    ("capacity = 4097", {"capacity": 4097, "workspace_bytes": ROOMY, "kv_q_bs": 2 * H * 4097 * 64, "kv_scale_bs": 2 * H * 4097}, (1, 1, 1)),
    ("head_dim = 128", {"head_dim": 128}, (1, 3, 1)),
    ("dtype F32", {"dtype": F32}, (3, 3, 3)),
    ("m = 0", {"m": 0}, (None, 1, None)),
    ("m = 9", {"m": 9, "workspace_bytes": ROOMY}, (None, 1, None)),
    ("m = -1", {"m": -1}, (None, 1, None)),
    ("B * m > 2^20", {"B": (1 << 18) + 1, "workspace_bytes": ROOMY}, (None, 1, None)),
    ("workspace one byte short", {"workspace_bytes": -1}, (1, 1, 1)),          # -1: the valid size less one
]
CASES = [(entry, name, fields, codes[i]) for name, fields, codes in FAULTS for i, entry in enumerate(ENTRIES) if codes[i] is not None]


@pytest.mark.parametrize("entry,rc", list(zip(ENTRIES, (3, 3, 1))))
def test_null_descriptor(entry, rc):
    assert _call(entry, None) == rc


@pytest.mark.parametrize("entry,name,fields,rc", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_one_broken_field(entry, name, fields, rc):
    d = _valid(entry)
    for f, v in fields.items():
        f = QKV_STRIDE[entry] if f == "qkv_stride" else f
        if not hasattr(d, f):
            assert f in ("kv_q_bs", "kv_scale_bs"), f          # the 16-bit entries have no such strides to enlarge
            continue
        setattr(d, f, d.workspace_bytes - 1 if (f, v) == ("workspace_bytes", -1) else v)
    assert _call(entry, d) == rc, name

