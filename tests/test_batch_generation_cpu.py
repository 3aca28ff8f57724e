"""CPU: the host side of several prompts on one decode graph -- plan_device_batch, that a decoder built without ragged=True
issues exactly the calls it always did, that a ragged one hands `first` to every layer's decode attention, and what the new
entry points refuse."""
import contextlib
import types

import pytest
import torch

from cogview_amd.generation import (DeviceGenerator, GraphDecoder, SamplingDecoder, decoder, generate_batch_on_device,
                                    plan_device_batch)
from tests.generation_cases import ToyIds


def _model(dtype=torch.float16, hidden=512, heads=8, layers=2):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


IDS = ToyIds(32, 16)
VOCAB = 56


def _seq(n_text, run, nb=1, marker="[BOI1]"):
    return [32 + (i % 16) for i in range(n_text)] + [IDS[marker]] + [-nb] * run


def test_plan_device_batch():
    plan = plan_device_batch([_seq(5, 20, 2), _seq(2, 20, 2), _seq(9, 20, 2)], IDS, VOCAB)
    assert plan["contexts"] == [6, 3, 10] and plan["P"] == 10 and plan["pads"] == [4, 7, 0]
    assert plan["run"] == 20 and plan["nb"] == 2 and plan["rows"] == 6 and plan["allow"] == (0, 32)
    assert plan["capacity"] == 64 and plan["offsets"] == [100000] * 3                       # 30 slots, rounded up to 64
    assert plan_device_batch([_seq(60, 5)], IDS, VOCAB)["capacity"] == 128                      # 66 slots
    # the [ROI2] offset may differ from row to row
    roi = [40, IDS["[ROI2]"], 41, IDS["[BOI1]"], -1, -1]
    assert plan_device_batch([roi, [40, 41, 42, IDS["[BOI1]"], -1, -1]], IDS, VOCAB)["offsets"] == [1, 100000]
    for seqs in ([_seq(5, 20), _seq(5, 21)],                                    # run lengths
                 [_seq(5, 20, 2), _seq(3, 20, 4)],                              # beam counts
                 [_seq(5, 20), _seq(5, 20, marker="[EOI1]")],                   # drawable ranges: image codes | text pieces
                 [_seq(5, 20), _seq(4000, 97)]):                                # 4098 slots
        with pytest.raises(NotImplementedError, match="generate_on_device"):
            plan_device_batch(seqs, IDS, VOCAB)


def test_default_decoder_is_unchanged(monkeypatch):
    """no `first` tensor, and decode_attention calls stubs of the OLD signature"""
    from cogview_amd import functional as F_
    from cogview_amd.mpu.transformer import StaticKV8Slot, StaticKVSlot
    for kv in (None, "e4m3"):
        dec = GraphDecoder(_model(), batch=2, capacity=64, **({} if kv is None else {"kv": kv}))
        assert dec.first is None and all(s.first is None for s in dec.slots)
        assert [k for k, t in vars(dec).items() if isinstance(t, torch.Tensor) and t.dtype == torch.int32] == ["table", "masked"]
    calls = []

    class Ops:
        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True):
            calls.append(("attention_decode", combine))
            return qkv

        @staticmethod
        def attention_decode_kv8(qkv, cache8, pos_index, heads, combine=True):
            calls.append(("attention_decode_kv8", combine))
            return qkv

    monkeypatch.setattr(F_, "ops", Ops)
    pos = torch.zeros(1, dtype=torch.long)
    s16 = StaticKVSlot(torch.zeros(1, 4, 128), pos, None)
    s8 = StaticKV8Slot(torch.zeros((1, 2, 1, 4, 64), dtype=torch.uint8), torch.ones((1, 2, 1, 4)), pos)
    for slot in (s16, s8):
        F_.decode_attention(torch.zeros(1, 1, 192), slot, 1)
        F_.decode_attention(torch.zeros(1, 1, 192), slot, 1, combine=False)
    assert calls == [("attention_decode", True), ("attention_decode", False), ("attention_decode_kv8", True), ("attention_decode_kv8", False)]


@pytest.mark.parametrize("kv", [None, "e4m3"])
@pytest.mark.parametrize("fused", [True, False])
def test_ragged_decoder_hands_first_to_every_layer(monkeypatch, kv, fused):
    from cogview_amd import functional as F_
    L_, V_, H_, NH_, B_ = 2, 64, 512, 8, 2
    m = _model()
    calls = []

    class Ops:
        @staticmethod
        def scalar_slab(slab):
            return contextlib.nullcontext()

        @staticmethod
        def gemv_ln(z, w, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            return torch.zeros(z.shape[0], w.shape[0], dtype=gamma.dtype), (torch.zeros(z.shape, dtype=torch.float32) if (post is not None and want_t) else None)

        @staticmethod
        def gemm(a, w, bias=None, **k):
            return torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype)

        @staticmethod
        def gemv_attn(parts, b, heads, cap, w, bias=None, absmax=None):
            return torch.zeros(b, w.shape[0], dtype=w.dtype)

        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True, first=None):
            calls.append(("attention_decode", combine, first))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

        @staticmethod
        def attention_decode_kv8(qkv, cache8, pos_index, heads, combine=True, first=None):
            calls.append(("attention_decode_kv8", combine, first))
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
    dec = GraphDecoder(m, batch=B_, capacity=64, ragged=True, **({} if kv is None else {"kv": kv}))
    assert dec.first.dtype == torch.int32 and dec.first.shape == (B_,) and not dec.first.any()
    assert all(s.first is dec.first for s in dec.slots)
    dec.fused = fused
    tr = m.transformer
    h0 = torch.zeros(B_, 1, H_, dtype=torch.float32)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    if not fused:
        monkeypatch.setattr(type(tr.final_layernorm), "forward", lambda self, x, residual=None: x.half())
        monkeypatch.setattr(F_, "tied_logits", lambda x, w: torch.zeros(B_, 1, V_, dtype=x.dtype))
    with torch.no_grad():
        logits = dec._step()
    assert logits.shape == (B_, 1, V_)
    name = "attention_decode" if kv is None else "attention_decode_kv8"
    assert [c[:2] for c in calls] == [(name, not fused)] * L_                 # the chain leaves the partials to the projection
    assert all(c[2] is dec.first for c in calls)
    assert isinstance(SamplingDecoder(m, batch=B_, capacity=64, ragged=True).first, torch.Tensor)
    assert SamplingDecoder(m, batch=B_, capacity=64).first is None


def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


def test_refusals(monkeypatch):
    seqs = [torch.tensor([40, IDS["[BOI1]"], -1, -1]), torch.tensor([40, 41, IDS["[BOI1]"], -1, -1])]
    m16, m32 = _model(), _model(torch.float32)
    from cogview_amd.mpu import initialize
    with monkeypatch.context() as mp:
        _no_alloc(mp)
        for kv in (None, "e4m3"):
            with pytest.raises(NotImplementedError, match="sparse generation.*filling_sequence"):
                generate_batch_on_device(None, seqs, _args(is_sparse=2), tokenizer=IDS, kv=kv)
            with pytest.raises(NotImplementedError, match="sparse generation.*filling_sequence"):
                DeviceGenerator(None, _args(is_sparse=2), rows=2, kv=kv)
        with pytest.raises(NotImplementedError, match="float32.*filling_sequence"):
            generate_batch_on_device(m32, seqs, _args(), tokenizer=IDS, kv="e4m3")
        with pytest.raises(NotImplementedError, match="float32.*filling_sequence"):
            DeviceGenerator(m32, _args(), rows=2, kv="e4m3")
        with pytest.raises(NotImplementedError, match="float32"):
            generate_batch_on_device(m32, seqs, _args(), tokenizer=IDS)
        with pytest.raises(NotImplementedError, match="float32"):
            GraphDecoder(m32, batch=2, ragged=True)
        mp.setattr(initialize, "mp_world_size_or_1", lambda: 2)
        for kv in (None, "e4m3"):
            with pytest.raises(NotImplementedError, match="model parallelism > 1.*filling_sequence"):
                generate_batch_on_device(None, seqs, _args(), tokenizer=IDS, kv=kv)
            with pytest.raises(NotImplementedError, match="model parallelism > 1.*filling_sequence"):
                DeviceGenerator(None, _args(), rows=2, kv=kv)
        with pytest.raises(NotImplementedError, match="model parallelism"):
            GraphDecoder(m16, batch=2, ragged=True)
    gen = DeviceGenerator(m16, _args(), rows=4, capacity=64)
    with pytest.raises(ValueError, match="built for 4"):
        gen(seqs, tokenizer=IDS)
    with pytest.raises(NotImplementedError, match="generate_on_device"):
        gen([torch.tensor([40, IDS["[BOI1]"]] + [-4] * 70)], tokenizer=IDS)
