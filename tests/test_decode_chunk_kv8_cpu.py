"""CPU: the host side of the chunk step on the 8-bit key/value cache -- the opt-in keyword kv_chunk on refuse_unsupported,
GraphDecoder, SamplingDecoder, DeviceFiller and DeviceBatchFiller (without it every refusal is what it was, before the first
allocation; with it chunk=C and kv="e4m3" build together), the slots' mark, which attention a step issues on recording stubs, and
the header entry."""
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import DeviceBatchFiller, DeviceFiller, GraphDecoder, SamplingDecoder, decoder
from tests.generation_cases import ToyIds
from tests.test_decode_chunk_cpu import _recording_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIE = NotImplementedError


def _model(dtype=torch.float16, layers=1, hidden=512, heads=8, vocab=64):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, vocab, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


@pytest.fixture(scope="module")
def model():
    return _model()


SITES = {"GraphDecoder": lambda m, **kw: GraphDecoder(m, **kw),
         "SamplingDecoder": lambda m, **kw: SamplingDecoder(m, **kw),
         "DeviceFiller": lambda m, **kw: DeviceFiller(m, _args(), **kw),
         "DeviceBatchFiller": lambda m, **kw: DeviceBatchFiller(m, _args(), rows=1, **kw)}


def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


# ------------------------------------------------------------------------------------------------------------------- the opt-in
@pytest.mark.parametrize("site", list(SITES))
@pytest.mark.parametrize("kw", [dict(chunk=4, kv="e4m3"), dict(chunk=4, kv="e4m3", kv_chunk=False)], ids=["default", "False"])
def test_without_the_keyword_the_pair_is_refused_as_before(monkeypatch, model, site, kw):
    _no_alloc(monkeypatch)
    with pytest.raises(NIE, match=r"chunk=4 with kv='e4m3': the 8-bit cache quantizes a key before it is attended, so it serves "
                                  r"one-token steps only -- use kv=None"):
        SITES[site](model, **kw)


@pytest.mark.parametrize("site", list(SITES))
@pytest.mark.parametrize("kw,exc,pat", [(dict(chunk=1), ValueError, "chunk=1"), (dict(chunk=9), ValueError, "chunk=9"),
                                        (dict(kv="int8", chunk=4), ValueError, "kv=")])
def test_the_keyword_leaves_the_other_limits(monkeypatch, model, site, kw, exc, pat):
    _no_alloc(monkeypatch)
    with pytest.raises(exc, match=pat):
        SITES[site](model, kv_chunk=True, **{**dict(kv="e4m3"), **kw})


def test_the_keyword_keeps_batch_times_chunk_at_eight(monkeypatch, model):
    m32 = _model(torch.float32)
    _no_alloc(monkeypatch)
    for build in (lambda: GraphDecoder(model, batch=2, chunk=8, kv="e4m3", kv_chunk=True),
                  lambda: SamplingDecoder(model, batch=3, chunk=4, kv="e4m3", kv_chunk=True),
                  lambda: DeviceBatchFiller(model, _args(), rows=4, chunk=4, kv="e4m3", kv_chunk=True)):
        with pytest.raises(ValueError, match="batch"):
            build()
    with pytest.raises(NIE, match="float32"):
        decoder.refuse_unsupported(None, "e4m3", model=m32, chunk=4, kv_chunk=True)


def test_refuse_unsupported_accepts_the_pair_only_with_the_keyword(model):
    with pytest.raises(NIE, match="kv=None"):
        decoder.refuse_unsupported(None, "e4m3", model=model, batch=1, chunk=4)
    assert decoder.refuse_unsupported(None, "e4m3", model=model, batch=1, chunk=4, kv_chunk=True) is None
    assert decoder.refuse_unsupported(None, "e4m3", model=model, batch=2, chunk=4, kv_chunk=True) is None
    # with kv=None or chunk=0 the keyword does nothing
    assert decoder.refuse_unsupported(None, None, model=model, batch=1, chunk=4, kv_chunk=True) is None
    assert decoder.refuse_unsupported(None, "e4m3", model=model, batch=1, kv_chunk=True) is None


# ------------------------------------------------------------------------------------------------------------------ the buffers
def _tensors(dec):
    return sorted(k for k, v in vars(dec).items() if isinstance(v, torch.Tensor))


@pytest.mark.parametrize("cls", [GraphDecoder, SamplingDecoder])
@pytest.mark.parametrize("batch,chunk", [(1, 8), (2, 4)])
def test_with_the_keyword_the_decoders_build(cls, batch, chunk):
    m = _model(layers=2)
    dec = cls(m, batch=batch, capacity=64, chunk=chunk, kv="e4m3", kv_chunk=True)
    assert dec.kv8 is not None and dec.caches is None and dec.chunk == chunk
    assert dec.kv8.q.shape == (2, batch, 2, 8, 64, 64) and dec.kv8.q.dtype == torch.uint8 and dec.kv8.scale.shape == (2, batch, 2, 8, 64)
    assert dec.tok_chunk.shape == dec.pos_chunk.shape == (batch, chunk) and dec.chunk_j.tolist() == list(range(chunk))
    assert dec.graph_chunk is None
    assert len(dec.slots) == 2 and all(s.chunk is True and s.pos_index is dec.pos_index for s in dec.slots)
    # the same tensors as the one-token 8-bit decoder plus the chunk buffers; the same allocations as without the mark
    plain8 = cls(m, batch=batch, capacity=64, kv="e4m3")
    assert sorted(set(_tensors(dec)) - set(_tensors(plain8))) == ["chunk_j", "pos_chunk", "tok_chunk"]
    assert [t.shape for t in dec.kv8.tensors()] == [t.shape for t in plain8.kv8.tensors()]
    assert all(s.chunk is False for s in plain8.slots)


def test_a_default_decoder_holds_no_new_tensors_and_the_keyword_alone_changes_nothing():
    m = _model()
    plain = GraphDecoder(m, batch=2, capacity=64)
    assert _tensors(plain) == ["masked", "pos", "pos_index", "slab", "table", "tok"] and plain.kv8 is None and len(plain.caches) == 1
    # kv_chunk=True with kv=None: the decoder it always built, with and without chunk=
    for kw in (dict(), dict(chunk=4)):
        a, b = GraphDecoder(m, batch=2, capacity=64, **kw), GraphDecoder(m, batch=2, capacity=64, kv_chunk=True, **kw)
        assert _tensors(a) == _tensors(b) and b.kv8 is None and [c.shape for c in a.caches] == [c.shape for c in b.caches]
        assert [type(s) for s in a.slots] == [type(s) for s in b.slots] and not any(hasattr(s, "chunk") for s in b.slots)
        assert sorted(vars(a)) == sorted(vars(b))
    # kv_chunk=True with chunk=0: the one-token 8-bit decoder, its slots unmarked
    c = GraphDecoder(m, batch=2, capacity=64, kv="e4m3", kv_chunk=True)
    assert c.chunk == 0 and not hasattr(c, "tok_chunk") and all(s.chunk is False for s in c.slots)


def test_the_cache_marks_its_slots_only_when_asked():
    from cogview_amd.mpu.transformer import KV8Cache, StaticKV8Slot
    pos = torch.zeros(1, dtype=torch.long)
    assert all(s.chunk is False for s in KV8Cache(2, 1, 2, 8, pos, "cpu").slots)
    marked = KV8Cache(2, 1, 2, 8, pos, "cpu", chunk=True)
    assert all(s.chunk is True for s in marked.slots) and [t.shape for t in marked.tensors()] == [(2, 1, 2, 2, 8, 64), (2, 1, 2, 2, 8)]
    assert StaticKV8Slot(marked.q[0], marked.scale[0], pos).chunk is False


# ---------------------------------------------------------------------------------------------- the keyword on the run drivers
def test_the_fillers_hand_the_keyword_on_only_where_it_is_set(monkeypatch, model):
    assert DeviceFiller(model, _args(), chunk=8).formats == dict(weights=None, chunk=8)
    assert DeviceFiller(model, _args(), kv="e4m3").formats == dict(weights=None, kv="e4m3")
    assert DeviceFiller(model, _args(), chunk=8, kv="e4m3", kv_chunk=True).formats == dict(weights=None, kv="e4m3", chunk=8, kv_chunk=True)
    assert DeviceBatchFiller(model, _args(), rows=2, chunk=4).formats == dict(weights=None, ragged=True, chunk=4)
    assert DeviceBatchFiller(model, _args(), rows=2, chunk=4, kv="e4m3", kv_chunk=True).formats == dict(
        weights=None, kv="e4m3", ragged=True, chunk=4, kv_chunk=True)
    # the refusal rule is called with the keyword only where it is set
    seen = []
    monkeypatch.setattr(decoder, "refuse_unsupported", lambda *a, **kw: seen.append(kw))
    DeviceFiller(model, _args(), chunk=8)
    DeviceFiller(model, _args(), chunk=8, kv="e4m3", kv_chunk=True)
    assert "kv_chunk" not in seen[0] and seen[1]["kv_chunk"] is True and "wide" not in seen[1]


def test_the_filler_builds_its_decoder_with_the_keyword(monkeypatch):
    ids = ToyIds(32, 16)
    model = types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8, dtype=torch.float16)))
    log = []

    class Fake:
        def __init__(self, model_, **kw):
            log.append(("ctor", kw))
            self.batch = kw["batch"]
            self.tok = torch.zeros((self.batch, 1), dtype=torch.long)
            self.graph = self.graph_chunk = self.offset = None

        def enable_sampling(self, *a, out_tokens=None, given=None, **kw):
            self.offset, self.scores, self.out_tokens = torch.zeros(1, dtype=torch.int64), torch.zeros(self.batch), out_tokens

        def start(self, tokens, position_ids, attention_mask=0):
            self.out_tokens.fill_(7)

        def capture(self):
            self.graph = self.graph_chunk = object()

        def generate(self, n, **kw):
            log.append(("generate", n, kw))

    monkeypatch.setattr(decoder, "SamplingDecoder", Fake)
    seq = [40, ids["[BOI1]"], -1, 3, 4, 5, -1, 6, -1, 9]
    f = DeviceFiller(model, _args(), capacity=64, chunk=4, kv="e4m3", kv_chunk=True)
    f(model, torch.tensor(seq), _args(), tokenizer=ids)
    assert log == [("ctor", dict(batch=1, capacity=64, weights=None, kv="e4m3", chunk=4, kv_chunk=True)), ("generate", 6, dict(widths=[4, 1, 1]))]
    assert f.model_calls == 3


# ------------------------------------------------------------------------------------------------------- the launch sequence
def _kv8_recording_ops(calls):
    """the recording stubs of test_decode_chunk_cpu with the two attentions of the 8-bit cache"""
    class Ops(_recording_ops(calls)):
        @staticmethod
        def attention_decode_kv8(qkv, cache8, pos_index, heads, combine=True, first=None):
            assert cache8.q.dtype == torch.uint8 and cache8.scale.dtype == torch.float32
            calls.append(("attention_decode_kv8", tuple(qkv.shape[:2]), combine))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype) if combine else "partials"

        @staticmethod
        def attention_decode_chunk_kv8(qkv, cache8, pos_index, heads, combine=True, first=None):
            assert cache8.chunk is True and cache8.q.dtype == torch.uint8 and cache8.scale.dtype == torch.float32
            calls.append(("attention_decode_chunk_kv8", tuple(qkv.shape[:2]), combine, cache8.q.data_ptr(), pos_index.data_ptr()))
            return torch.zeros(qkv.shape[0], qkv.shape[1], heads * 64, dtype=qkv.dtype) if combine else "partials"
    return Ops


def _stubbed(monkeypatch, m, H_, fuse):
    from cogview_amd import functional as F_
    calls = []
    ops_ = _kv8_recording_ops(calls)
    monkeypatch.setattr(F_, "ops", ops_)
    monkeypatch.setattr(decoder, "ops", ops_)
    monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", fuse)
    monkeypatch.setattr(F_, "mp_world_size_or_1", lambda: 1)

    def embed(self, tok, pos, emb):
        h = torch.zeros(*tok.shape, H_)
        h._cogv_absmax = torch.ones(1)
        return h
    monkeypatch.setattr(type(m.transformer), "embed", embed)
    return calls


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_chunk_step_issues_the_8bit_chunk_attention_once_per_layer(monkeypatch, fuse):
    """GraphDecoder(chunk=C, kv="e4m3", kv_chunk=True)._step_chunk on stubs: 4 rows take the chain, 8 rows run layer by layer; both
    issue attention_decode_chunk_kv8 once per layer on the layer's own slot.  _step still issues attention_decode_kv8."""
    L_, V_, H_, NH_ = 2, 64, 512, 8
    m = _model(layers=L_, hidden=H_, heads=NH_, vocab=V_)
    calls = _stubbed(monkeypatch, m, H_, fuse)
    dec4 = GraphDecoder(m, batch=1, capacity=128, chunk=4, kv="e4m3", kv_chunk=True)
    with torch.no_grad():
        assert dec4._step_chunk().shape == (1, 4, V_)
    names = [c[0] for c in calls if c[0] != "new_absmax_slot"]
    assert names[:2] == ["gemv_ln", "attention_decode_chunk_kv8"] and "sandwich_ln_fwd" not in names, "4 rows: the chain"
    att = [c for c in calls if c[0].startswith("attention")]
    assert att == [("attention_decode_chunk_kv8", (1, 4), fuse == "0", s.q.data_ptr(), dec4.pos_index.data_ptr()) for s in dec4.slots]
    assert len([c for c in calls if c[0] == "gemv_attn"]) == (L_ if fuse == "1" else 0)
    assert all(s.out is s.q for s in dec4.slots)
    del calls[:]
    with torch.no_grad():
        assert dec4._step().shape == (1, 1, V_)
    assert [c for c in calls if c[0].startswith("attention")] == [("attention_decode_kv8", (1, 1), fuse == "0")] * L_
    del calls[:]
    dec8 = GraphDecoder(m, batch=1, capacity=128, chunk=8, kv="e4m3", kv_chunk=True)
    with torch.no_grad():
        assert dec8._step_chunk().shape == (1, 8, V_)
    names = [c[0] for c in calls if c[0] != "new_absmax_slot"]
    per_layer = ["sandwich_ln_fwd", "gemm", "attention_decode_chunk_kv8", "gemm", "sandwich_ln_fwd", "sandwich_ln_fwd", "gemm", "gemm", "sandwich_ln_fwd"]
    assert names == per_layer * L_ + ["sandwich_ln_fwd", "gemm"], "8 rows: layer by layer"
    att = [c for c in calls if c[0].startswith("attention")]
    assert att == [("attention_decode_chunk_kv8", (1, 8), True, s.q.data_ptr(), dec8.pos_index.data_ptr()) for s in dec8.slots]
    del calls[:]
    with torch.no_grad():
        assert dec8._step().shape == (1, 1, V_)
    assert [c for c in calls if c[0].startswith("attention")] == [("attention_decode_kv8", (1, 1), fuse == "0")] * L_


def test_decode_attention_routes_by_the_slots_mark(monkeypatch):
    from cogview_amd import functional as F_
    from cogview_amd.mpu.transformer import StaticKV8Slot
    calls = []
    monkeypatch.setattr(F_, "ops", _kv8_recording_ops(calls))
    q, s, pos = torch.zeros((1, 2, 1, 4, 64), dtype=torch.uint8), torch.ones((1, 2, 1, 4)), torch.zeros(1, dtype=torch.long)
    plain, marked = StaticKV8Slot(q, s, pos), StaticKV8Slot(q, s, pos, chunk=True)
    with pytest.raises(NIE, match="the 8-bit key/value cache serves one-token decode steps only: use kv=None for chunk steps"):
        F_.decode_attention(torch.zeros(1, 2, 192), plain, 1)
    assert not calls
    assert F_.decode_attention(torch.zeros(1, 2, 192), marked, 1).shape == (1, 2, 64) and marked.out is q
    assert F_.decode_attention(torch.zeros(1, 2, 192), marked, 1, combine=False) == "partials"
    assert F_.decode_attention(torch.zeros(1, 1, 192), marked, 1).shape == (1, 1, 64)          # one token: the one-token op
    assert [c[:3] for c in calls] == [("attention_decode_chunk_kv8", (1, 2), True), ("attention_decode_chunk_kv8", (1, 2), False),
                                      ("attention_decode_kv8", (1, 1), True)]


# -------------------------------------------------------------------------------------------------------------------- the header
def test_binding_mirrors_the_header():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_attn_decode_chunk_kv8_desc \{(.*?)\} cogv_attn_decode_chunk_kv8_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part.split("[")[0])[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.AttnDecodeChunkKv8Desc._fields_]
    # placed after cogv_attention_decode_kv8, with a comment that cites the reference call site
    assert src.index("int cogv_attention_decode_kv8(") < src.index("typedef struct cogv_attn_decode_chunk_kv8_desc") < src.index("int cogv_attention_decode_chunk_kv8(")
    head = src[:src.index("typedef struct cogv_attn_decode_chunk_kv8_desc")]
    assert "generation/sampling.py:139-148" in head[head.rindex("/*"):]
    assert _lib.lib().cogv_attention_decode_chunk_kv8(None, None) == 3
