"""CPU: the host side of the 8-bit decode weights -- what weights="e4m3" refuses, that the keyword reaches the decoder from
generate_on_device and DeviceFiller, and that the new header entries follow tests/test_abi.py's conventions."""
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import DeviceFiller, GraphDecoder, SamplingDecoder, decoder, generate_on_device
from tests.generation_cases import ToyIds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cogv_quantize_rows_e4m3", "cogv_gemm_w8", "cogv_gemv_ln_w8", "cogv_gemv_attn_w8")


def _model(dtype=torch.float16, hidden=512, heads=8):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(1, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


def test_decoder_refuses_what_the_8bit_step_does_not_cover(monkeypatch):
    with pytest.raises(ValueError, match="weights="):
        GraphDecoder(_model(), weights="int8")
    with pytest.raises(NotImplementedError, match="float32"):
        GraphDecoder(_model(torch.float32), weights="e4m3")
    with pytest.raises(NotImplementedError, match="contraction length"):
        GraphDecoder(_model(hidden=320, heads=5), weights="e4m3")            # h % 512 != 0
    with pytest.raises(NotImplementedError, match="rows"):
        GraphDecoder(_model(), batch=9, weights="e4m3")
    from cogview_amd.mpu import initialize
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: 2)
    with pytest.raises(NotImplementedError, match="model parallelism"):
        SamplingDecoder(_model(), weights="e4m3")


def test_callers_refuse_before_the_model_is_touched(monkeypatch):
    seq = torch.tensor([1, 2, -1, -1])
    for kw, exc, pat in ((dict(is_sparse=2), NotImplementedError, "sparse"), (dict(), ValueError, "weights=")):
        w = "e4m3" if kw else "fp4"
        with pytest.raises(exc, match=pat):
            generate_on_device(None, seq, _args(**kw), weights=w)
        with pytest.raises(exc, match=pat):
            DeviceFiller(None, _args(**kw), weights=w)
    from cogview_amd.mpu import initialize
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: 2)
    with pytest.raises(NotImplementedError, match="model parallelism"):
        generate_on_device(None, seq, _args(), weights="e4m3")
    with pytest.raises(NotImplementedError, match="model parallelism"):
        DeviceFiller(None, _args(), weights="e4m3")


def test_keyword_reaches_the_decoder(monkeypatch):
    seen = []

    class Stop(Exception):
        pass

    class Spy:
        def __init__(self, model, batch=1, capacity=1152, weights=None):
            seen.append((batch, weights))
            raise Stop

    monkeypatch.setattr(decoder, "SamplingDecoder", Spy)
    ids = ToyIds(32, 16)
    model = types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8)))
    seq = torch.tensor([40, ids["[BOI1]"], -3, -3, -3])
    for w in (None, "e4m3"):
        with pytest.raises(Stop):
            generate_on_device(model, seq, _args(), tokenizer=ids, weights=w)
        f = DeviceFiller(model, _args(), weights=w)
        with pytest.raises(Stop):
            f(model, torch.tensor([40, ids["[BOI1]"], -1, 3, -1]), _args(), tokenizer=ids)
    assert seen == [(3, None), (1, None), (3, "e4m3"), (1, "e4m3")]


def test_default_decoder_allocates_nothing_for_8bit_weights():
    dec = GraphDecoder(_model(), batch=1, capacity=64)
    assert dec.w8 is None


def test_new_header_entries_follow_the_abi_conventions():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, bare), name                 # declared, returning the error code
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert res is _lib._i and len(args) == len(decl.split(",")), name       # one ctypes argument per C parameter
        assert args[-1] is _lib._vp and decl.split(",")[-1].strip() == "void* stream"
    # each entry cites the reference call site it serves (a file:line under the reference tree) in the comment in front of it
    for name in NEW:
        head = src[:src.index("int %s(" % name)]
        comment = head[head.rindex("/*"):]
        assert re.search(r"[a-z_/]+\.py:\d+", comment), name
    # the new struct mirrors the header's field order; the existing ones keep their layout
    body = re.search(r"typedef struct cogv_w8_weight \{(.*?)\} cogv_w8_weight;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.W8Weight._fields_]
    assert [f[0] for f in _lib.GemmDesc._fields_][-1] == "dropout_row0" and len(_lib.GemmDesc._fields_) == 27
    # argument errors come back as codes without a device: null pointers -> 1 (bad argument)
    assert lib.cogv_quantize_rows_e4m3(0, None, 8, 1, 8, None, 8, None, None) == 1
    assert lib.cogv_gemm_w8(None, None, None) == 1


@pytest.mark.parametrize("fused", [True, False])
def test_8bit_step_launch_sequence_on_recording_stubs(monkeypatch, fused):
    """GraphDecoder(weights="e4m3")._step on stubs (no GPU): every Linear product of the step is an 8-bit one reading the
    (q, scale) pair quantized from ITS weight, the 16-bit products are never called, and the embedding lookup keeps the
    16-bit table; fused: the chain's five launches per layer, else layer by layer with the Sandwich-LN launches."""
    from cogview_amd import functional as F_
    L_, V_, H_, NH_, B_ = 2, 64, 512, 8, 2
    from cogview_amd.model import GPT2Model
    m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, 32, 32, False).half().eval()
    calls, quantized = [], {}

    def _q(w):
        q, s = torch.zeros(w.shape, dtype=torch.uint8), torch.ones(w.shape[0])
        quantized[id(q)] = w
        return q, s

    def _src(qs):
        return tuple(quantized[id(qs[0])].shape)

    class Ops:
        quantize_rows_e4m3 = staticmethod(_q)

        @staticmethod
        def scalar_slab(slab):
            import contextlib
            return contextlib.nullcontext()

        @staticmethod
        def gemv_ln_w8(z, qs, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            calls.append(("gemv_ln_w8", _src(qs), gelu))
            out = torch.zeros(z.shape[0], qs[0].shape[0], dtype=gamma.dtype)
            return out, (torch.zeros(z.shape, dtype=torch.float32) if (post is not None and want_t) else None)

        @staticmethod
        def gemm_w8(a, qs, bias=None, gelu=False, absmax=None):
            calls.append(("gemm_w8", _src(qs), gelu))
            return torch.zeros(a.shape[0], qs[0].shape[0], dtype=a.dtype)

        @staticmethod
        def gemv_attn_w8(parts, b, heads, cap, qs, dtype, bias=None, absmax=None):
            calls.append(("gemv_attn_w8", _src(qs), False))
            return torch.zeros(b, qs[0].shape[0], dtype=dtype)

        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True):
            calls.append(("attention_decode", combine))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

        @staticmethod
        def sandwich_ln_fwd(x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
            calls.append(("ln",))
            return torch.zeros(x.shape, dtype=torch.float32 if residual is not None else gamma.dtype), None, None

        @staticmethod
        def new_absmax_slot(dev):
            return torch.zeros(1)

        @staticmethod
        def gemm(*a, **k):
            raise AssertionError("a 16-bit product inside the 8-bit step")

        gemv_ln = gemv_attn = gemm

    monkeypatch.setattr(F_, "ops", Ops)
    monkeypatch.setattr(decoder, "ops", Ops)
    monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", "1")
    dec = GraphDecoder(m, batch=B_, capacity=64, weights="e4m3")
    assert len(quantized) == 4 * L_ + 1 and _src(dec.w8.emb) == (V_, H_)
    dec.fused = fused
    tr = m.transformer
    h0 = torch.zeros(B_, 1, H_, dtype=torch.float32)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    logits = dec._step()
    assert logits.shape == (B_, 1, V_)
    shapes = [c[1] for c in calls if c[0].endswith("_w8")]
    assert shapes == [(3 * H_, H_), (H_, H_), (4 * H_, H_), (H_, 4 * H_)] * L_ + [(V_, H_)]
    assert [c[2] for c in calls if c[0].endswith("_w8")] == [False, False, True, False] * L_ + [False]
    names = [c[0] for c in calls]
    if fused:
        assert names == ["gemv_ln_w8", "attention_decode", "gemv_attn_w8", "gemv_ln_w8", "gemm_w8"] * L_ + ["gemv_ln_w8"]
        assert ("attention_decode", False) in calls
    else:
        assert names == ["ln", "gemm_w8", "attention_decode", "gemm_w8", "ln", "ln", "gemm_w8", "gemm_w8", "ln"] * L_ + ["ln", "gemm_w8"]
