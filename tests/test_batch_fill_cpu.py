"""CPU: the host side of super-resolution for several images on one decode graph -- the `given_stride` field of
cogv_sample_desc (header, ctypes mirror, the host check), generation.plan_device_batch_fill over magnify-shaped windows of
different text lengths and over magnify's nine windows, what DeviceBatchFiller asks of its decoder (on a recording fake), what it
refuses before the first allocation, and magnify_batch against magnify on a deterministic stub filler."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import (DeviceBatchFiller, decoder, magnify, magnify_batch, plan_chunk_steps, plan_device_batch_fill,
                                    plan_device_fill)
from tests.generation_cases import ToyIds
from tests.test_device_fill_cpu import MIDFIX, magnify_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIE = NotImplementedError


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


# ------------------------------------------------------------------------------------------------------------------ the struct
def test_given_stride_sits_in_front_of_given():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_sample_desc \{(.*?)\} cogv_sample_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert re.fullmatch(r"int64_t\s+given_stride", decls[-2]), decls[-2]
    assert re.fullmatch(r"const\s+int64_t\s*\*\s*given", decls[-1]), decls[-1]
    assert _lib.SampleDesc._fields_[-2] == ("given_stride", C.c_int64)
    assert _lib.SampleDesc._fields_[-1] == ("given", C.c_void_p)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for d in decls for part in d.split(",")]
    assert names == [f[0] for f in _lib.SampleDesc._fields_]


@pytest.mark.parametrize("stride", [-1, 1, 15])
def test_a_bad_given_stride_is_a_bad_argument(stride):
    """refused on the host, before any launch: the pointers are never followed"""
    d = _lib.SampleDesc()
    d.dtype, d.rows, d.vocab, d.row_stride = 0, 3, 64, 64
    d.logits = d.pos_index = d.counter = d.given = 4096
    d.temperature, d.top_k, d.top_p, d.allow_lo, d.allow_hi = 1.0, 0, 0.0, 0, 64
    d.capacity = 16
    d.given_stride = stride
    assert _lib.lib().cogv_sample_logits(C.byref(d), None) == 1


# -------------------------------------------------------------------------------------------------------------------- the plan
IDS = ToyIds(8192, 500)
VOCAB = 8704


def _window(n_text, lines=3, given_lines=2, seed=0):
    """a magnify-shaped window as a list: text, a 16 x 16 patch, the marker run, `lines` lines of 32 codes whose first 16 are
    given in the first `given_lines` lines (those of line 0 join the context, the later ones lie inside the run); text, patch and
    given ids drawn from `seed`"""
    g = torch.Generator().manual_seed(seed)
    text = (8192 + torch.randint(0, 500, (n_text,), generator=g)).tolist()
    patch = torch.randint(0, 8192, (256,), generator=g).tolist()
    target = torch.full((lines, 32), -1, dtype=torch.long)
    target[:given_lines, :16] = torch.randint(0, 8192, (given_lines, 16), generator=g)
    return text + patch + [IDS[m] for m in MIDFIX] + target.reshape(-1).tolist()


def test_plan_of_three_windows_with_different_text_lengths():
    seqs = [_window(6, seed=1), _window(4, seed=2), _window(2, seed=3)]
    singles = [plan_device_fill(s, IDS, VOCAB) for s in seqs]
    plan = plan_device_batch_fill(seqs, IDS, VOCAB)
    assert plan["contexts"] == [283, 281, 279] and plan["P"] == 283 and plan["pads"] == [0, 2, 4]
    assert plan["replays"] == 79 == singles[0]["replays"] and plan["run"] == 80 and plan["nb"] == 1 and plan["rows"] == 3
    assert plan["allow"] == (0, 8192) and plan["capacity"] == 384 and plan["trailing"] == [0, 0, 0]
    assert plan["offsets"] == [6 + 256 + 1, 4 + 256 + 1, 2 + 256 + 1]
    assert len({tuple(s[-64:-48]) for s in seqs}) == 3                     # the rows' given ids differ
    for row, single, pad, seq in zip(plan["given"], singles, plan["pads"], seqs):
        want = [-1] * 384
        for i, t in enumerate(single["given"]):
            want[pad + i] = t
        assert row == want
        assert [t for t in row if t >= 0] == seq[-64:-48] and row[pad + len(seq) - 64] == seq[-64]     # line 1's first 16 codes
    assert plan["pattern"] == [0 if t >= 0 else -1 for t in plan["given"][0]]
    for C_ in (0, 2, 4, 8):
        widths = plan_chunk_steps(plan["pattern"], plan["P"], plan["replays"], C_)
        for single in singles:
            assert widths == plan_chunk_steps(single["given"], single["context"], single["replays"], C_)
    assert plan_device_batch_fill(seqs[:1], IDS, VOCAB)["pads"] == [0]


@pytest.mark.parametrize("C_,calls", [(0, 6039), (2, 5063), (4, 4575)])
def test_plan_over_the_nine_magnify_windows_of_two_images(C_, calls):
    a = magnify_windows(IDS, [8192 + 5, 8192 + 17, 8192 + 3], seed=0)
    b = magnify_windows(IDS, [8192 + 7] * 7, seed=1)
    total = 0
    for (_, sa), (_, sb) in zip(a, b):
        plan = plan_device_batch_fill([sa, sb], IDS, VOCAB)
        assert plan["pads"] == [4, 0] and plan["capacity"] <= 1408
        total += len(plan_chunk_steps(plan["pattern"], plan["P"], plan["replays"], C_))
    assert total == calls


# ------------------------------------------------------------------------------------------------ the decoder calls, on a fake
TOY = ToyIds(32, 16)
BOI1, EOI1 = TOY["[BOI1]"], TOY["[EOI1]"]


def _stub_model(dtype=torch.float16):
    return types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8, dtype=dtype)))


def test_batch_filler_trace(monkeypatch):
    model, log = _stub_model(), []

    class Fake:
        def __init__(self, model_, **kw):
            log.append(("ctor", kw))
            self.batch = kw["batch"]
            self.tok = torch.zeros((self.batch, 1), dtype=torch.long)
            self.graph = self.graph_chunk = self.offset = None

        def enable_sampling(self, *a, out_tokens=None, out_base=0, given=None, **kw):
            log.append(("enable_sampling", tuple(out_tokens.shape), out_base, tuple(given.shape)))
            self.offset, self.scores = torch.zeros(1, dtype=torch.int64), torch.zeros(self.batch)
            self.out_tokens, self.given = out_tokens, given

        def start_ragged(self, tokens, position_ids, pads):
            log.append(("start_ragged", tokens.tolist(), position_ids.tolist(), list(pads), self.given[:, :8].tolist()))
            self.out_tokens.copy_(100 * torch.arange(self.batch).view(-1, 1) + torch.arange(self.out_tokens.shape[1]).view(1, -1))
            self.scores.copy_(-torch.arange(1, self.batch + 1).float())

        def capture(self):
            log.append(("capture",))
            self.graph = self.graph_chunk = object()

        def generate(self, n, **kw):
            log.append(("generate", n, kw))

    monkeypatch.setattr(decoder, "SamplingDecoder", Fake)
    seqs = [torch.tensor([40, 41, BOI1, -1, 3, 4, 5, -1, 9]), torch.tensor([42, BOI1, -1, 6, 7, 8, -1, 10])]
    f = DeviceBatchFiller(model, _args(), rows=3, capacity=64, seed=2)
    assert log == [] and f.dec is None
    rows = f(seqs, tokenizer=TOY)
    assert log == [("ctor", dict(batch=3, capacity=64, weights=None, ragged=True)),
                   ("enable_sampling", (3, 64), 0, (3, 64)),
                   # the table is on the device before the prefill: per row, by slot; the spare row repeats the last sequence
                   ("start_ragged", [[40, 41, BOI1], [0, 42, BOI1], [0, 42, BOI1]], [[0, 1, 2], [0, 0, 1], [0, 0, 1]], [0, 1, 1],
                    [[-1, -1, -1, -1, 3, 4, 5, -1], [-1, -1, -1, -1, 6, 7, 8, -1], [-1, -1, -1, -1, 6, 7, 8, -1]]),
                   ("capture",), ("generate", 4, {})]
    # column = slot: row g's run is out[g, P : P + replays + 1]; the trailing given id comes from the input
    assert [r.tolist() for r in rows] == [[[40, 41, BOI1, 3, 4, 5, 6, 7, 9]], [[42, BOI1, 103, 104, 105, 106, 107, 10]]]
    assert f.scores.tolist() == [-1.0, -2.0] and f.model_calls == 4
    # a chunk filler hands the widths of the shared pattern on
    del log[:]
    fc = DeviceBatchFiller(model, _args(), rows=2, capacity=64, chunk=4)
    fc(seqs, tokenizer=TOY)
    assert log[0] == ("ctor", dict(batch=2, capacity=64, weights=None, ragged=True, chunk=4))
    assert log[-1] == ("generate", 4, dict(widths=[4])) and fc.model_calls == 1
    with pytest.raises(NIE, match="DeviceFiller"):
        fc([torch.tensor([40, BOI1] + [-1] * 63)], tokenizer=TOY)                     # 65 slots in a filler of 64


# ------------------------------------------------------------------------------------------------------------------- refusals
def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


def _t(*ids):
    return torch.tensor(list(ids))


PLAN_REFUSALS = [("given patterns", [_t(40, BOI1, -1, 3, -1), _t(40, BOI1, -1, -1, -1)], NIE, "DeviceFiller"),
                 ("replays", [_t(40, BOI1, -1, -1), _t(40, BOI1, -1, -1, -1)], NIE, "DeviceFiller"),
                 ("drawable range", [_t(40, BOI1, -1, -1), _t(40, EOI1, -1, -1)], NIE, "DeviceFiller"),
                 ("nb > 1", [_t(40, BOI1, -2, -2), _t(40, BOI1, -2, -2)], NIE, "filling_sequence"),
                 ("4096 slots", [_t(*([40, BOI1] + [-1] * 4200))], NIE, "4096"),
                 ("G > rows", [_t(40, BOI1, -1, -1)] * 3, ValueError, "3 sequences")]


@pytest.mark.parametrize("seqs,exc,pat", [pytest.param(*r[1:], id=r[0]) for r in PLAN_REFUSALS])
def test_a_call_refuses_before_the_first_allocation(monkeypatch, seqs, exc, pat):
    f = DeviceBatchFiller(_stub_model(), _args(), rows=2, capacity=64)
    _no_alloc(monkeypatch)
    with pytest.raises(exc, match=pat):
        f(seqs, tokenizer=TOY)
    assert f.dec is None


def test_the_plan_refusals_themselves():
    for _, seqs, exc, pat in PLAN_REFUSALS[:5]:
        with pytest.raises(exc, match=pat):
            plan_device_batch_fill([s.tolist() for s in seqs], TOY, 56)
    with pytest.raises(ValueError):
        plan_device_batch_fill([], TOY, 56)


CTOR_REFUSALS = [("is_sparse=2", {}, dict(is_sparse=2), "m16", 1, NIE, "sparse generation.*filling_sequence"),
                 ("is_sparse=1", {}, dict(is_sparse=1), "m16", 1, ValueError, "is_sparse==2"),
                 ("mp=2", {}, {}, "m16", 2, NIE, "model parallelism > 1.*filling_sequence"),
                 ("float32", {}, {}, "m32", 1, NIE, "float32"),
                 ("bad weights", dict(weights="fp4"), {}, "m16", 1, ValueError, "weights="),
                 ("bad kv", dict(kv="int8"), {}, "m16", 1, ValueError, "kv="),
                 ("rows=4,chunk=4", dict(rows=4, chunk=4), {}, "m16", 1, ValueError, "batch"),
                 ("chunk,kv", dict(chunk=2, kv="e4m3"), {}, "m16", 1, NIE, "kv=None")]


@pytest.mark.parametrize("kw,akw,model,mp,exc,pat", [pytest.param(*r[1:], id=r[0]) for r in CTOR_REFUSALS])
def test_the_constructor_refuses_before_the_first_allocation(monkeypatch, kw, akw, model, mp, exc, pat):
    from cogview_amd.mpu import initialize
    m = _stub_model(torch.float16 if model == "m16" else torch.float32)
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: mp)
    _no_alloc(monkeypatch)
    with pytest.raises(exc, match=pat):
        DeviceBatchFiller(m, _args(**akw), **{**dict(rows=2), **kw})


def test_a_call_with_sparse_args_is_refused(monkeypatch):
    f = DeviceBatchFiller(_stub_model(), _args(), rows=2, capacity=64)
    _no_alloc(monkeypatch)
    with pytest.raises(NIE, match="sparse generation.*filling_sequence"):
        f([_t(40, BOI1, -1, -1)], args=_args(is_sparse=2), tokenizer=TOY)


# -------------------------------------------------------------------------------------------------------------- magnify_batch
def _stub_fill(model, seq, args, invalid_slices=None, tokenizer=None):
    """fills every mark with a hash of its position and the row's text"""
    l = seq.tolist()
    text = l[:l.index(tokenizer["[EOI1]"]) - 256]
    out = seq.clone()
    for i, t in enumerate(l):
        if t < 0:
            out[i] = (31 * i + 7 * sum(text) + 3) % tokenizer.img_tokenizer.num_tokens
    return out.unsqueeze(0)


def test_magnify_batch_is_magnify_per_image():
    g = torch.Generator().manual_seed(9)
    codes = torch.randint(0, 8192, (3, 1024), generator=g)
    texts = [8192 + torch.randint(0, 500, (n,), generator=g) for n in (6, 3, 1)]
    calls = []

    def fill(seqs, args, tokenizer=None):
        calls.append(len(seqs))
        return [_stub_fill(None, s, args, tokenizer=tokenizer) for s in seqs]

    big = magnify_batch(None, IDS, codes, texts, _args(), fill=fill)
    assert calls == [3] * 9 and big.shape == (3, 4096) and int(big.min()) >= 0
    for g_, (code, text) in enumerate(zip(codes, texts)):
        assert torch.equal(big[g_:g_ + 1], magnify(None, IDS, code, text, _args(), fill=_stub_fill))
    assert len({tuple(r.tolist()) for r in big}) == 3
    as_list = magnify_batch(None, IDS, list(codes), texts, _args(), fill=fill)
    assert torch.equal(as_list, big)
    with pytest.raises(ValueError):
        magnify_batch(None, IDS, codes, texts[:2], _args(), fill=fill)
