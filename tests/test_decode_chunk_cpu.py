"""CPU: the host side of the multi-token decode step -- generation.plan_chunk_steps over magnify's nine windows, what chunk=C
refuses (before the first allocation, on GraphDecoder, SamplingDecoder and DeviceFiller), which tensors a decoder holds with and
without it, how the keyword and the planned widths reach the decoder, and the launch sequence of a chunk step on recording
stubs."""
import contextlib
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import (DeviceFiller, GraphDecoder, IdSpace, SamplingDecoder, decoder, plan_chunk_steps,
                                    plan_device_fill)
from tests.generation_cases import ToyIds
from tests.test_device_fill_cpu import magnify_windows


def _model(dtype=torch.float16, layers=1, hidden=512, heads=8, vocab=64):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, vocab, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


# ------------------------------------------------------------------------------------------------------------------- the plan
def _check_widths(widths, given, context, replays, C):
    assert sum(widths) == replays and set(widths) <= {1, C}
    i = context
    for w in widths:
        if w > 1:
            assert all(t >= 0 for t in given[i + 1:i + w]) and i + w <= context + replays
        elif C > 1 and i + C <= context + replays:               # greedy: a single step only where a chunk does not fit
            assert any(t < 0 for t in given[i + 1:i + C])
        i += w


@pytest.mark.parametrize("space", ["released", "toy"])
@pytest.mark.parametrize("C,calls,chunks", [(0, 6039, 0), (2, 5063, 976), (4, 4575, 488), (8, 4331, 244)])
def test_plan_over_the_nine_magnify_windows(space, C, calls, chunks):
    ids = IdSpace() if space == "released" else ToyIds(8192, 500)
    vocab = 58240 if space == "released" else 8704
    n_img = ids.img_tokenizer.num_tokens
    total = n_chunks = 0
    for _, seq in magnify_windows(ids, [n_img + 5, n_img + 17, n_img + 3]):
        p = plan_device_fill(seq, ids, vocab)
        widths = plan_chunk_steps(p["given"], p["context"], p["replays"], C)
        _check_widths(widths, p["given"], p["context"], p["replays"], C)
        total += len(widths)
        n_chunks += sum(1 for w in widths if w > 1)
    assert (total, n_chunks) == (calls, chunks)


def test_plan_edge_cases():
    g = lambda marks: [-1 if m == "." else 7 for m in marks]
    # context 2; inputs at positions 2 ... 2 + replays - 1
    assert plan_chunk_steps(g("xx.xxx.."), 2, 5, 4) == [4, 1]                # positions 3, 4, 5 given: one chunk from the first replay
    assert plan_chunk_steps(g("xx.xx..."), 2, 5, 4) == [1] * 5               # a run shorter than C - 1
    assert plan_chunk_steps(g("xx.xx..."), 2, 5, 3) == [3, 1, 1]
    assert plan_chunk_steps(g("xx..xxx."), 2, 5, 4) == [1, 4]                # a run reaching the last mark: the chunk ends at it
    assert plan_chunk_steps(g("xx..xxx."), 2, 4, 4) == [1, 1, 1, 1]          # ... and does not run past the replays
    assert plan_chunk_steps(g("xx.xxxxxxx."), 2, 8, 4) == [4, 4]             # the given id that ends a chunk starts the next one
    assert plan_chunk_steps(g("xx.xxx.."), 2, 5, 0) == [1] * 5 == plan_chunk_steps(g("xx.xxx.."), 2, 5, 1)
    assert plan_chunk_steps(g("xx."), 2, 0, 8) == []


# ------------------------------------------------------------------------------------------------------------------- refusals
def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


NIE = NotImplementedError
REFUSALS = [("chunk=1", dict(chunk=1), "m16", 1, ValueError, "chunk=1"),
            ("chunk=9", dict(chunk=9), "m16", 1, ValueError, "chunk=9"),
            ("batch=2,chunk=8", dict(batch=2, chunk=8), "m16", 1, ValueError, "batch"),
            ("kv", dict(chunk=4, kv="e4m3"), "m16", 1, NIE, "kv=None"),
            ("float32", dict(chunk=4), "m32", 1, NIE, "float32"),
            ("mp=2", dict(chunk=4), "m16", 2, NIE, "model parallelism"),
            ("weights,float32", dict(chunk=4, weights="e4m3"), "m32", 1, NIE, "float32")]


@pytest.fixture(scope="module")
def models():
    return {"m16": _model(), "m32": _model(torch.float32)}


SITES = {"GraphDecoder": GraphDecoder, "SamplingDecoder": SamplingDecoder,
         "DeviceFiller": lambda model, **kw: DeviceFiller(model, _args(), **kw)}


# (a filler has one row: no batch keyword)
@pytest.mark.parametrize("site,kw,model,mp,exc,pat", [pytest.param(site, *r[1:], id=f"{site}-{r[0]}") for site in SITES for r in REFUSALS
                                                       if not (site == "DeviceFiller" and "batch" in r[1])])
def test_refusals_come_before_the_first_allocation(monkeypatch, models, site, kw, model, mp, exc, pat):
    from cogview_amd.mpu import initialize
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: mp)
    _no_alloc(monkeypatch)
    with pytest.raises(exc, match=pat):
        SITES[site](models[model], **kw)


def test_refusal_of_8bit_weights_asks_the_plan_at_the_chunk_rows(monkeypatch):
    from cogview_amd import functional as F_
    asked = []
    monkeypatch.setattr(F_, "w8_decode_supported", lambda tr, rows: asked.append(rows))
    decoder.refuse_unsupported("e4m3", model=_model(), batch=2, chunk=4)
    assert asked == [2, 8]
    monkeypatch.setattr(F_, "w8_decode_supported", lambda tr, rows: "no class" if rows == 8 else None)
    with pytest.raises(NIE, match="weights='e4m3': no class"):
        decoder.refuse_unsupported("e4m3", model=_model(), batch=2, chunk=4)


# ---------------------------------------------------------------------------------------------------------------- the buffers
def _tensors(dec):
    return sorted(k for k, v in vars(dec).items() if isinstance(v, torch.Tensor))


def test_default_decoder_holds_no_new_tensors_and_chunk_allocates_its_buffers():
    m = _model()
    plain = GraphDecoder(m, batch=2, capacity=64)
    assert _tensors(plain) == ["masked", "pos", "pos_index", "slab", "table", "tok"] and plain.chunk == 0
    assert not hasattr(plain, "tok_chunk") and not hasattr(plain, "graph_chunk")
    with pytest.raises(AssertionError, match="chunk="):
        plain.step_chunk(torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long))
    dec = GraphDecoder(m, batch=2, capacity=64, chunk=4)
    assert sorted(set(_tensors(dec)) - set(_tensors(plain))) == ["chunk_j", "pos_chunk", "tok_chunk"]
    assert dec.tok_chunk.shape == dec.pos_chunk.shape == (2, 4) and dec.tok_chunk.dtype == dec.pos_chunk.dtype == torch.long
    assert dec.chunk_j.tolist() == [0, 1, 2, 3] and dec.graph_chunk is None
    s = SamplingDecoder(m, batch=1, capacity=64, chunk=8)
    assert s.chunk == 8 and s.chunk_steps == 0 and isinstance(s.chunk_steps, int) and s.tok_chunk.shape == (1, 8)
    assert SamplingDecoder(m, batch=1, capacity=64).chunk_steps == 0


# ------------------------------------------------------------------------------------------------- keyword and widths on a fake
def test_filler_hands_the_keyword_and_the_planned_widths_to_its_decoder(monkeypatch):
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
    f = DeviceFiller(model, _args(), capacity=64, chunk=4)
    row = f(model, torch.tensor(seq), _args(), tokenizer=ids)
    assert log == [("ctor", dict(batch=1, capacity=64, weights=None, chunk=4)), ("generate", 6, dict(widths=[4, 1, 1]))]
    assert f.model_calls == 3 and row.tolist() == [[40, ids["[BOI1]"], 7, 7, 7, 7, 7, 7, 7, 9]]
    # a re-arm drops both graphs
    dec = f.dec
    f(model, torch.tensor(seq), _args(temperature=0.5), tokenizer=ids)
    assert dec.graph is not None and log[-1] == ("generate", 6, dict(widths=[4, 1, 1]))
    del log[:]
    # chunk=0: the calls a filler always made
    f0 = DeviceFiller(model, _args(), capacity=64)
    f0(model, torch.tensor(seq), _args(), tokenizer=ids)
    assert log == [("ctor", dict(batch=1, capacity=64, weights=None)), ("generate", 6, {})] and f0.model_calls == 6


# ------------------------------------------------------------------------------------------------------- the launch sequence
class _Slot:
    def __init__(self, b, h):
        self.cache = torch.zeros(b, 128, 2 * h, dtype=torch.float16)
        self.pos_index = torch.zeros((), dtype=torch.int64)
        self.out = None
        self.capacity = 128


def _recording_ops(calls):
    class Ops:
        @staticmethod
        def scalar_slab(slab):
            return contextlib.nullcontext()

        @staticmethod
        def gemv_ln(z, w, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            calls.append(("gemv_ln", z.shape[0], tuple(w.shape), z_absmax is None, post is not None, gelu, absmax is None))
            out = torch.zeros(z.shape[0], w.shape[0], dtype=w.dtype)
            return out, (torch.zeros(z.shape, dtype=torch.float32) if (post is not None and want_t) else None)

        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True):
            calls.append(("attention_decode", tuple(qkv.shape[:2]), combine))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype) if combine else "partials"

        @staticmethod
        def attention_decode_chunk(qkv, cache, pos_index, heads, combine=True, first=None):
            calls.append(("attention_decode_chunk", tuple(qkv.shape[:2]), combine))
            return torch.zeros(qkv.shape[0], qkv.shape[1], heads * 64, dtype=qkv.dtype) if combine else "partials"

        @staticmethod
        def gemm(a, b, bias=None, absmax=None, **kw):
            calls.append(("gemm", a.shape[0], tuple(b.shape), absmax is None))
            return torch.zeros(a.shape[0], b.shape[0], dtype=b.dtype)

        @staticmethod
        def gemv_attn(parts, batch, heads, capacity, w, bias=None, absmax=None):
            calls.append(("gemv_attn", batch, tuple(w.shape), absmax is None))
            assert parts == "partials"
            return torch.zeros(batch, w.shape[0], dtype=w.dtype)

        @staticmethod
        def sandwich_ln_fwd(x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
            calls.append(("sandwich_ln_fwd", tuple(x.shape[:2]), residual is not None))
            return torch.zeros(x.shape, dtype=torch.float32 if residual is not None else gamma.dtype), None, None

        @staticmethod
        def new_absmax_slot(dev):
            calls.append(("new_absmax_slot",))
            return torch.zeros(1)
    return Ops


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_decode_chain_of_a_chunk_issues_the_one_token_sequence_on_four_rows(monkeypatch, fuse):
    """functional.decode_chain with h0 [1, 4, h]: launch for launch what it issues for h0 [4, 1, h] (four cache rows, one token
    each), with attention_decode_chunk on qkv [1, 4, 3h] in the attention slot; the Sandwich contract holds (z_absmax=None after
    layer 0, no abs-max slots)."""
    from cogview_amd import functional as F_
    L_, V_, H_, NH_ = 3, 256, 512, 8
    m = _model(layers=L_, hidden=H_, heads=NH_, vocab=V_)
    seqs = {}
    for name, (b, s) in {"chunk": (1, 4), "rows": (4, 1)}.items():
        calls = []
        monkeypatch.setattr(F_, "ops", _recording_ops(calls))
        monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", fuse)
        slots = [_Slot(b, H_) for _ in range(L_)]
        logits = F_.decode_chain(m.transformer, torch.zeros(b, s, H_), torch.ones(1), slots, m.word_embeddings.weight)
        assert logits.shape == (b, s, V_) and all(sl.out is sl.cache for sl in slots)
        seqs[name] = calls
    assert not [c for c in seqs["chunk"] if c[0] == "new_absmax_slot"]
    att = [c for c in seqs["chunk"] if c[0].startswith("attention")]
    assert att == [("attention_decode_chunk", (1, 4), fuse == "0")] * L_
    assert [c for c in seqs["rows"] if c[0].startswith("attention")] == [("attention_decode", (4, 1), fuse == "0")] * L_
    strip = lambda cs: [c if not c[0].startswith("attention") else ("attention", c[2]) for c in cs]
    assert strip(seqs["chunk"]) == strip(seqs["rows"]) and len(seqs["chunk"]) == 5 * L_ + 1
    for li in range(L_):
        qkv_launch = seqs["chunk"][5 * li]
        assert qkv_launch[:3] == ("gemv_ln", 4, (3 * H_, H_)) and qkv_launch[3] == (li > 0), "z_absmax=None after layer 0"
    assert all(c[1] == 4 for c in seqs["chunk"] if c[0] in ("gemv_ln", "gemm", "gemv_attn"))


def test_chunk_step_of_eight_rows_runs_layer_by_layer(monkeypatch):
    """GraphDecoder(chunk=8)._step_chunk on stubs: 8 rows are above the chain's row limit, so every Sandwich-LN is its own launch
    on [1, 8, h], the products are plain ones on 8 rows and the attention is the chunk op with its combine; chunk=4 takes the
    chain.  The one-token step of the same decoder is untouched (attention_decode on one row)."""
    from cogview_amd import functional as F_
    L_, V_, H_, NH_ = 2, 64, 512, 8
    m = _model(layers=L_, hidden=H_, heads=NH_, vocab=V_)
    calls = []
    ops_ = _recording_ops(calls)
    monkeypatch.setattr(F_, "ops", ops_)
    monkeypatch.setattr(decoder, "ops", ops_)
    monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", "0")
    monkeypatch.setattr(F_, "mp_world_size_or_1", lambda: 1)
    tr = m.transformer

    def embed(self, tok, pos, emb):
        h = torch.zeros(*tok.shape, H_)
        h._cogv_absmax = torch.ones(1)
        return h
    monkeypatch.setattr(type(tr), "embed", embed)
    dec = GraphDecoder(m, batch=1, capacity=128, chunk=8)
    with torch.no_grad():
        logits = dec._step_chunk()
    assert logits.shape == (1, 8, V_)
    names = [c[0] for c in calls if c[0] != "new_absmax_slot"]
    per_layer = ["sandwich_ln_fwd", "gemm", "attention_decode_chunk", "gemm", "sandwich_ln_fwd", "sandwich_ln_fwd", "gemm", "gemm", "sandwich_ln_fwd"]
    assert names == per_layer * L_ + ["sandwich_ln_fwd", "gemm"]
    assert all(c[1] == (1, 8) for c in calls if c[0] == "sandwich_ln_fwd") and all(c[1] == 8 for c in calls if c[0] == "gemm")
    assert [c for c in calls if c[0].startswith("attention")] == [("attention_decode_chunk", (1, 8), True)] * L_
    del calls[:]
    dec4 = GraphDecoder(m, batch=1, capacity=128, chunk=4)
    with torch.no_grad():
        assert dec4._step_chunk().shape == (1, 4, V_)
    assert [c[0] for c in calls][:3] == ["gemv_ln", "attention_decode_chunk", "gemm"] and "sandwich_ln_fwd" not in [c[0] for c in calls]
    del calls[:]
    with torch.no_grad():
        assert dec4._step().shape == (1, 1, V_)
    assert [c for c in calls if c[0].startswith("attention")] == [("attention_decode", (1, 1), True)] * L_


def test_8bit_cache_has_no_chunk_form():
    from cogview_amd import functional as F_
    from cogview_amd.mpu.transformer import StaticKV8Slot
    s8 = StaticKV8Slot(torch.zeros((1, 2, 1, 4, 64), dtype=torch.uint8), torch.ones((1, 2, 1, 4)), torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="kv=None"):
        F_.decode_attention(torch.zeros(1, 2, 192), s8, 1)


def test_binding_mirrors_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_attn_decode_chunk_desc \{(.*?)\} cogv_attn_decode_chunk_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part.split("[")[0])[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.AttnDecodeChunkDesc._fields_]
    assert [f[0] for f in _lib.AttnDecodeDesc._fields_][-1] == "first" and len(_lib.AttnDecodeDesc._fields_) == 18
    lib = _lib.lib()
    assert lib.cogv_attention_decode_chunk(None, None) == 3
    # the comment in front of the descriptor cites the reference call site, as its neighbours do
    head = src[:src.index("typedef struct cogv_attn_decode_chunk_desc")]
    assert "generation/sampling.py:139-148" in head[head.rindex("/*"):]
