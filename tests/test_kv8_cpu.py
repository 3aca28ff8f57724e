"""CPU: the host side of the 8-bit key/value cache -- what kv="e4m3" refuses, that the keyword reaches the decoder, which
attention call each slot type makes in the decode step's three forms, the prefill's broadcast, and the new header entries."""
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import DeviceFiller, GraphDecoder, SamplingDecoder, decoder, generate_on_device
from tests.generation_cases import ToyIds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cogv_kv_quantize_e4m3", "cogv_attention_decode_kv8")


def _model(dtype=torch.float16, hidden=512, heads=8, layers=1):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


def test_decoder_refuses_what_the_8bit_cache_does_not_cover(monkeypatch):
    m16, m32 = _model(), _model(torch.float32)
    from cogview_amd.mpu import initialize
    with monkeypatch.context() as mp:
        _no_alloc(mp)
        with pytest.raises(ValueError, match="kv="):
            GraphDecoder(m16, kv="int8")
        with pytest.raises(NotImplementedError, match="float32"):
            GraphDecoder(m32, kv="e4m3")
        mp.setattr(initialize, "mp_world_size_or_1", lambda: 2)
        with pytest.raises(NotImplementedError, match="model parallelism"):
            SamplingDecoder(m16, kv="e4m3")


def test_callers_refuse_before_the_model_is_touched(monkeypatch):
    seq = torch.tensor([1, 2, -1, -1])
    m32 = _model(torch.float32)
    from cogview_amd.mpu import initialize
    with monkeypatch.context() as mp:
        _no_alloc(mp)
        for kw, kv, exc, pat in ((dict(is_sparse=2), "e4m3", NotImplementedError, "sparse.*filling_sequence"), (dict(), "fp4", ValueError, "kv=")):
            with pytest.raises(exc, match=pat):
                generate_on_device(None, seq, _args(**kw), kv=kv)
            with pytest.raises(exc, match=pat):
                DeviceFiller(None, _args(**kw), kv=kv)
        with pytest.raises(NotImplementedError, match="float32.*filling_sequence"):
            generate_on_device(m32, seq, _args(), kv="e4m3")
        with pytest.raises(NotImplementedError, match="float32.*filling_sequence"):
            DeviceFiller(m32, _args(), kv="e4m3")
        mp.setattr(initialize, "mp_world_size_or_1", lambda: 2)
        with pytest.raises(NotImplementedError, match="model parallelism.*filling_sequence"):
            generate_on_device(None, seq, _args(), kv="e4m3")
        with pytest.raises(NotImplementedError, match="model parallelism.*filling_sequence"):
            DeviceFiller(None, _args(), kv="e4m3")


def test_keyword_reaches_the_decoder(monkeypatch):
    seen = []

    class Stop(Exception):
        pass

    class Spy:
        def __init__(self, model, batch=1, capacity=1152, **kw):
            seen.append((batch, kw))
            raise Stop

    monkeypatch.setattr(decoder, "SamplingDecoder", Spy)
    ids = ToyIds(32, 16)
    model = types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8, dtype=torch.float16)))
    seq = torch.tensor([40, ids["[BOI1]"], -3, -3, -3])
    for w, kv in ((None, None), (None, "e4m3"), ("e4m3", "e4m3")):
        with pytest.raises(Stop):
            generate_on_device(model, seq, _args(), tokenizer=ids, weights=w, kv=kv)
        f = DeviceFiller(model, _args(), weights=w, kv=kv)
        with pytest.raises(Stop):
            f(model, torch.tensor([40, ids["[BOI1]"], -1, 3, -1]), _args(), tokenizer=ids)
    # the default issues the call it always did: no kv keyword at all
    assert seen == [(3, dict(weights=None)), (1, dict(weights=None)),
                    (3, dict(weights=None, kv="e4m3")), (1, dict(weights=None, kv="e4m3")),
                    (3, dict(weights="e4m3", kv="e4m3")), (1, dict(weights="e4m3", kv="e4m3"))]


def test_cache_allocation_by_keyword():
    m = _model(layers=2)
    dec = GraphDecoder(m, batch=2, capacity=64)
    assert dec.kv8 is None and len(dec.caches) == 2 and dec.caches[0].shape == (2, 64, 1024)
    assert not [t for t in vars(dec).values() if isinstance(t, torch.Tensor) and t.dtype == torch.uint8]
    dec = GraphDecoder(m, batch=2, capacity=64, kv="e4m3")
    assert dec.caches is None and dec.kv8.q.shape == (2, 2, 2, 8, 64, 64) and dec.kv8.q.dtype == torch.uint8
    assert dec.kv8.scale.shape == (2, 2, 2, 8, 64) and dec.kv8.scale.dtype == torch.float32
    assert [s.q.data_ptr() for s in dec.slots] == [dec.kv8.q[i].data_ptr() for i in range(2)]
    assert all(s.pos_index is dec.pos_index and s.capacity == 64 for s in dec.slots)
    assert dec.kv8.q.numel() + 4 * dec.kv8.scale.numel() == 2 * 2 * 64 * 8 * 136          # 136 bytes per (slot, head): keys and values, 68 each


def test_dequantize_restates_the_16bit_layout():
    from cogview_amd.mpu.transformer import StaticKV8Slot
    g = torch.Generator().manual_seed(1)
    b, H, cap = 2, 3, 5
    q = torch.randint(0, 0x7E, (b, 2, H, cap, 64), dtype=torch.uint8, generator=g)
    scale = torch.rand((b, 2, H, cap), generator=g) + 0.5
    out = StaticKV8Slot(q, scale, None).dequantize()
    assert out.shape == (b, cap, 2 * H * 64) and out.dtype == torch.float32
    for (bi, plane, head, slot) in ((0, 0, 0, 0), (1, 1, 2, 4), (1, 0, 1, 3)):
        want = q[bi, plane, head, slot].view(torch.float8_e4m3fn).float() * scale[bi, plane, head, slot]
        assert torch.equal(out[bi, slot, (plane * H + head) * 64:(plane * H + head + 1) * 64], want)


def test_other_consumers_of_an_8bit_slot_raise():
    from cogview_amd.mpu.transformer import StaticKV8Slot
    m = _model()
    slot = StaticKV8Slot(torch.zeros((1, 2, 8, 16, 64), dtype=torch.uint8), torch.ones((1, 2, 8, 16)), torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="8-bit"):
        slot.append(torch.zeros(1, 2, 512), torch.zeros(1, 2, 512))
    with pytest.raises(NotImplementedError, match="8-bit"):                    # the gathered multi-token / op-by-op form
        m.transformer.layers[0].attention(torch.zeros(1, 1, 512, dtype=torch.float16), 0, mem=slot)


def test_prefill_broadcasts_a_one_row_prefill(monkeypatch):
    """_prefill on stubs: the quantizer is called once per layer on the prefill's memories (1 row), writes cache row 0, and the
    bytes and scales of the filled slots are copied into the other rows; other slots stay as they were."""
    from cogview_amd.mpu import transformer as T
    m = _model(layers=2)
    B, cap, n, H = 3, 16, 5, 8
    dec = GraphDecoder(m, batch=B, capacity=cap, kv="e4m3")
    calls = []

    class Ops:
        @staticmethod
        def kv_quantize_e4m3(kv, q, scale, slot0=0):
            calls.append((tuple(kv.shape), tuple(q.shape), slot0))
            rows = kv.shape[0]
            q[:, :, :, slot0:slot0 + kv.shape[1]] = 7 + len(calls)
            scale[:, :, :, slot0:slot0 + kv.shape[1]] = 0.5 * len(calls)

    monkeypatch.setattr(T, "ops", Ops)
    mems = [torch.zeros(1, n, 2 * H * 64, dtype=torch.float16) for _ in range(2)]
    monkeypatch.setattr(type(dec.gpt), "__call__", lambda self, *a, **k: (torch.zeros(1, n, 64), *mems))
    dec._prefill(torch.zeros(1, n, dtype=torch.long), torch.zeros(1, n, dtype=torch.long), 0)
    assert calls == [((1, n, 2 * H * 64), (1, 2, H, cap, 64), 0)] * 2 and dec.length == n
    for i, slot in enumerate(dec.slots):
        assert bool((slot.q[:, :, :, :n] == 8 + i).all()) and bool((slot.scale[:, :, :, :n] == 0.5 * (i + 1)).all())
        assert not slot.q[:, :, :, n:].any() and bool((slot.scale[:, :, :, n:] == 1.0).all())
    # B rows: quantized in place, nothing to broadcast
    calls.clear()
    mems = [torch.zeros(B, n, 2 * H * 64, dtype=torch.float16) for _ in range(2)]
    dec._prefill(torch.zeros(B, n, dtype=torch.long), torch.zeros(B, n, dtype=torch.long), 0)
    assert calls == [((B, n, 2 * H * 64), (B, 2, H, cap, 64), 0)] * 2


@pytest.mark.parametrize("kv", [None, "e4m3"])
@pytest.mark.parametrize("form", ["chain", "chain_w8", "layers_w8", "layers"])
def test_attention_call_by_slot_type(monkeypatch, kv, form):
    """GraphDecoder._step on recording stubs: an 8-bit slot makes decode_chain, _decode_chain_w8, decode_layers_w8 and the
    layer-by-layer 16-bit-weight path call attention_decode_kv8 where they called attention_decode, with the same combine flags;
    a 16-bit slot calls attention_decode(qkv, slot.cache, slot.pos_index, heads[, combine=False]) as before."""
    from cogview_amd import functional as F_
    from cogview_amd.model import GPT2Model
    L_, V_, H_, NH_, B_ = 2, 64, 512, 8, 2
    m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, 32, 32, False).half().eval()
    calls = []

    class Ops:
        @staticmethod
        def quantize_rows_e4m3(w):
            return torch.zeros(w.shape, dtype=torch.uint8), torch.ones(w.shape[0])

        @staticmethod
        def scalar_slab(slab):
            import contextlib
            return contextlib.nullcontext()

        @staticmethod
        def gemv_ln(z, w, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            return torch.zeros(z.shape[0], w.shape[0], dtype=gamma.dtype), (torch.zeros(z.shape, dtype=torch.float32) if (post is not None and want_t) else None)

        @staticmethod
        def gemv_ln_w8(z, qs, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            return Ops.gemv_ln(z, qs[0], bias, gamma, beta, eps, z_absmax, post, residual, want_t)

        @staticmethod
        def gemm(a, w, bias=None, **k):
            return torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype)

        @staticmethod
        def gemm_w8(a, qs, bias=None, gelu=False, absmax=None):
            return torch.zeros(a.shape[0], qs[0].shape[0], dtype=a.dtype)

        @staticmethod
        def gemv_attn(parts, b, heads, cap, w, bias=None, absmax=None):
            calls.append(("gemv_attn", cap))
            return torch.zeros(b, w.shape[0], dtype=w.dtype)

        @staticmethod
        def gemv_attn_w8(parts, b, heads, cap, qs, dtype, bias=None, absmax=None):
            calls.append(("gemv_attn_w8", cap))
            return torch.zeros(b, qs[0].shape[0], dtype=dtype)

        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True):
            assert isinstance(cache, torch.Tensor) and cache.shape == (B_, 64, 2 * H_)
            calls.append(("attention_decode", combine, cache.data_ptr(), pos_index.data_ptr(), heads))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

        @staticmethod
        def attention_decode_kv8(qkv, cache8, pos_index, heads, combine=True):
            assert cache8.q.shape == (B_, 2, NH_, 64, 64) and cache8.scale.shape == (B_, 2, NH_, 64)
            calls.append(("attention_decode_kv8", combine, cache8.q.data_ptr(), pos_index.data_ptr(), heads))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

        @staticmethod
        def sandwich_ln_fwd(x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
            return torch.zeros(x.shape, dtype=torch.float32 if residual is not None else gamma.dtype), None, None

        @staticmethod
        def new_absmax_slot(dev):
            return torch.zeros(1)

    monkeypatch.setattr(F_, "ops", Ops)
    monkeypatch.setattr(decoder, "ops", Ops)
    monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", "1")
    monkeypatch.setattr(F_, "mp_world_size_or_1", lambda: 1)
    monkeypatch.setattr(F_, "mp_rank_or_0", lambda: 0)
    w8 = form.endswith("_w8")
    dec = GraphDecoder(m, batch=B_, capacity=64, weights="e4m3" if w8 else None, **({} if kv is None else {"kv": kv}))
    dec.fused = form.startswith("chain")
    tr = m.transformer
    h0 = torch.zeros(B_, 1, H_, dtype=torch.float32)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    if form == "layers":
        monkeypatch.setattr(type(tr.final_layernorm), "forward", lambda self, x, residual=None: x.half())
        monkeypatch.setattr(F_, "tied_logits", lambda x, w: torch.zeros(B_, 1, V_, dtype=x.dtype))
    with torch.no_grad():
        logits = dec._step()
    assert logits.shape == (B_, 1, V_)
    name = "attention_decode" if kv is None else "attention_decode_kv8"
    combine = not dec.fused                                 # the chain leaves the partials to the projection's prologue
    ptrs = [(s.cache if kv is None else s.q).data_ptr() for s in dec.slots]
    att = [c for c in calls if c[0].startswith("attention_decode")]
    assert att == [(name, combine, p, dec.pos_index.data_ptr(), NH_) for p in ptrs]
    proj = [c for c in calls if c[0].startswith("gemv_attn")]
    assert proj == ([("gemv_attn_w8" if w8 else "gemv_attn", 64)] * L_ if dec.fused else [])
    assert all(s.out is (s.cache if kv is None else s.q) for s in dec.slots)


def test_new_header_entries_follow_the_abi_conventions():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, bare), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert res is _lib._i and len(args) == len(decl.split(",")), name
        assert args[-1] is _lib._vp and decl.split(",")[-1].strip() == "void* stream"
        head = src[:src.index("int %s(" % name)]
        assert re.search(r"[a-z_/]+\.py:\d+", head[head.rindex("/*"):]), name   # the reference call site it serves
    body = re.search(r"typedef struct cogv_attn_decode_kv8_desc \{(.*?)\} cogv_attn_decode_kv8_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.AttnDecodeKv8Desc._fields_]
    # the fields of cogv_attn_decode_desc, with `cache` (and its strides) replaced by the bytes, the scales and a batch stride each
    old = [f[0] for f in _lib.AttnDecodeDesc._fields_]
    i = old.index("cache")
    assert names == old[:i] + ["kv_q", "kv_q_bs", "kv_scale", "kv_scale_bs"] + old[i + 3:]
    # argument errors come back as codes without a device
    assert lib.cogv_kv_quantize_e4m3(0, None, 0, 0, 1, 1, 1, None, 0, None, 0, 1, 0, None) == 1
    assert lib.cogv_attention_decode_kv8(None, None) == 1
    d = _lib.AttnDecodeKv8Desc()
    d.dtype, d.B, d.H, d.capacity, d.head_dim = 0, 1, 1, 128, 32
    assert lib.cogv_attention_decode_kv8(d, None) == 1                     # head_dim != 64
    d.head_dim, d.qkv, d.kv_q, d.kv_scale, d.pos, d.workspace, d.out = 64, 4096, 4096 + 8, 4096, 4096, 4096, 4096
    d.kv_q_bs, d.kv_scale_bs, d.workspace_bytes = 2 * 128 * 64, 2 * 128, 1 << 20
    assert lib.cogv_attention_decode_kv8(d, None) == 1                     # bytes not 16-byte aligned
    d.kv_q, d.kv_scale = 4096, 4096 + 2
    assert lib.cogv_attention_decode_kv8(d, None) == 1                     # scales not 4-byte aligned
    d.kv_scale, d.workspace_bytes = 4096, 16
    assert lib.cogv_attention_decode_kv8(d, None) == 1                     # short workspace
    d.workspace_bytes, d.dtype = 1 << 20, 2
    assert lib.cogv_attention_decode_kv8(d, None) == 3                     # fp32: unsupported
