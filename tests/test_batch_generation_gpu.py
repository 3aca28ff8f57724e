"""GPU: several prompts on ONE decode graph -- generate_batch_on_device and DeviceGenerator (SamplingDecoder(ragged=True): the
contexts right-aligned in the caches, one `first` slot per cache row).

Prompts on the toy golden model (tests/generation_cases.py; h = 256: the step runs layer by layer): A is the golden t2i_seq, B is
A with three of its five text pieces removed between [ROI1] and [BASE], C is A with five extra text pieces inserted there.
The fused chain and the 8-bit weight stream need h % 512 == 0, so those cases run on the model of tests/test_kv8_decode_gpu.py
(2 layers, h = 1024) with contexts of 8, 5 and 13 ids."""
import types

import pytest
import torch

from cogview_amd.generation import (DeviceGenerator, add_interlacing_beam_marks, generate_batch_on_device, generate_on_device)
from tests.generation_cases import COIN_FLIP, ToyIds, build_model, check_tokens, load_golden

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def _golden(golden_dir):
    if not _GOLDEN:
        z, c = load_golden(golden_dir)
        ids = ToyIds(c["img_tokens"], c["txt_tokens"])
        _GOLDEN["v"] = (z, c, ids, build_model(z, c, "cuda", True))
    return _GOLDEN["v"]


def _prompts(z, c, nb):
    """A, B, C as device tensors with -nb marks"""
    a = z["t2i_seq"].tolist()
    assert a[6:8] == [c["img_tokens"] + c["txt_tokens"] + 1, c["img_tokens"] + c["txt_tokens"] + 2]        # [BASE] [BOI1]
    extra = [c["img_tokens"] + t for t in (3, 141, 59, 265, 358)]
    seqs = [a, a[:3] + a[6:], a[:4] + extra + a[4:]]
    out = []
    for s in seqs:
        t = torch.tensor(s, dtype=torch.long, device="cuda")
        add_interlacing_beam_marks(t, nb=nb)
        out.append(t)
    return out


def _greedy():
    return types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)


def _sampled():
    return types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)


@pytest.mark.parametrize("capture", [True, False])
def test_greedy_batch_of_three_prompts(golden_dir, capture):
    z, c, ids, model = _golden(golden_dir)
    seqs = _prompts(z, c, 1)
    outs, scores = generate_batch_on_device(model, [s.clone() for s in seqs], _greedy(), tokenizer=ids, capture=capture)
    assert len(outs) == 3 and scores.shape == (3, 1) and scores.dtype == torch.float32
    for seq, out in zip(seqs, outs):
        assert out.shape == (1, seq.numel())
        assert torch.equal(out[0][seq >= 0], seq[seq >= 0])
    check_tokens(outs[0].expand(c["beams"], -1).cpu(), z, c)          # the golden's two greedy beams are one row twice
    # every row alone and unpadded through the full forward (the rule of test_teacher_forced_consistency)
    for seq, out in zip(seqs, outs):
        n = int((seq >= 0).sum())
        pos = torch.arange(out.shape[1], device="cuda").unsqueeze(0)
        with torch.no_grad():
            logits, *_ = model(out, pos, 0, None, None, 0)
        x = logits[0, n - 1:-1].float()
        x[..., c["img_tokens"]:] = -float("inf")
        std = x[..., :c["img_tokens"]].std(dim=-1)
        top = torch.topk(x, 2, dim=-1)
        gap = (top[0][..., 0] - top[0][..., 1]) / std
        gen = out[0, n:]
        ok = (gen == top[1][..., 0]) | (gap < COIN_FLIP)
        print(f"context {n}: smallest top-2 gap {float(gap.min()):.4f} std, {int((gen != top[1][..., 0]).sum())} ids off the arg-max")
        assert ok.all(), (n, gap[~ok].tolist())


def _h1024(dtype=torch.float16):
    from tests.test_kv8_decode_gpu import _model
    from tests.test_w8_decode_gpu import N_IMG, N_TXT
    ids = ToyIds(N_IMG, N_TXT)
    g = torch.Generator().manual_seed(9)
    text = (N_IMG + torch.randint(0, N_TXT, (11,), generator=g)).tolist()
    tail = [ids["[BASE]"], ids["[BOI1]"]]
    return _model(dtype), ids, [text[:6] + tail, text[:3] + tail, text + tail], N_IMG


def _h1024_seqs(ctxs, which, nb, run=16):
    out = []
    for i in which:
        t = torch.tensor(ctxs[i] + [-1] * run, dtype=torch.long, device="cuda")
        add_interlacing_beam_marks(t, nb=nb)
        out.append(t)
    return out


def _captured_equals_eager(model, ids, seqs, n_img, nb, **formats):
    res = [generate_batch_on_device(model, [s.clone() for s in seqs], _sampled(), tokenizer=ids, seed=1234, capture=cap, **formats)
           for cap in (True, False)]
    (outs, scores), (outs_e, scores_e) = res
    assert scores.shape == (len(seqs), nb) and torch.isfinite(scores).all()
    assert torch.equal(scores, scores_e)
    for seq, out, out_e in zip(seqs, outs, outs_e):
        assert torch.equal(out, out_e), (out.tolist(), out_e.tolist())
        n = int((seq >= 0).sum())
        assert out.shape == (nb, seq.numel()) and torch.equal(out[:, :n], seq[:n].expand(nb, n))
        assert int(out[:, n:].min()) >= 0 and int(out[:, n:].max()) < n_img
        if nb > 1:
            assert len({tuple(r) for r in out[:, n:].tolist()}) > 1, "independent rows drew identical sequences"
    return outs, scores


@pytest.mark.parametrize("which,nb", [((0, 1, 2), 1), ((1, 2), 4)])
def test_captured_batch_equals_eager(which, nb):
    """3 prompts x 1: the fused chain (<= 4 rows); 2 prompts x 4: eight rows, layer by layer"""
    from cogview_amd import functional as F_
    model, ids, ctxs, n_img = _h1024()
    tr = model.module.transformer
    assert F_.decode_chain_supported(tr, len(which) * nb) == (len(which) * nb <= 4)
    _captured_equals_eager(model, ids, _h1024_seqs(ctxs, which, nb), n_img, nb)


@pytest.mark.parametrize("formats", [dict(kv="e4m3"), dict(weights="e4m3"), dict(kv="e4m3", weights="e4m3")],
                         ids=["kv8", "w8", "kv8+w8"])
def test_captured_batch_equals_eager_in_8_bits(formats):
    model, ids, ctxs, n_img = _h1024()
    _captured_equals_eager(model, ids, _h1024_seqs(ctxs, (1, 2), 4), n_img, 4, **formats)


def test_device_generator_reuse(golden_dir):
    """[C, C], then [B, A] on the same decoder and graph: a shorter prompt set after a longer one (stale slots past it, other
    pads) gives what a fresh decoder gives"""
    z, c, ids, model = _golden(golden_dir)
    a, b, cc = _prompts(z, c, 1)
    gen = DeviceGenerator(model, _greedy(), rows=2, capacity=64)
    outs0, _ = gen([cc.clone(), cc.clone()], tokenizer=ids)
    assert torch.equal(outs0[0], outs0[1])
    graph = gen.dec.graph
    assert graph is not None
    outs, scores = gen([b.clone(), a.clone()], tokenizer=ids)
    assert gen.dec.graph is graph
    want, want_scores = generate_batch_on_device(model, [b.clone(), a.clone()], _greedy(), tokenizer=ids)
    assert all(torch.equal(o, w) for o, w in zip(outs, want)), ([o.tolist() for o in outs], [w.tolist() for w in want])
    assert torch.equal(scores, want_scores)


def test_device_generator_rearm(golden_dir):
    """a sampled call on [C, C], then a greedy one on [B, A] through the same generator: other sampler values re-arm the sampler and
    capture again while a graph exists, and give what a fresh decoder gives (top_k = 1: the draws do not depend on the generator
    offset the re-arm keeps)"""
    z, c, ids, model = _golden(golden_dir)
    a, b, cc = _prompts(z, c, 1)
    gen = DeviceGenerator(model, _sampled(), rows=2, capacity=64)
    gen([cc.clone(), cc.clone()], tokenizer=ids)
    graph = gen.dec.graph
    assert graph is not None
    outs, scores = gen([b.clone(), a.clone()], args=_greedy(), tokenizer=ids)
    assert gen.dec.graph is not None and gen.dec.graph is not graph
    want, want_scores = generate_batch_on_device(model, [b.clone(), a.clone()], _greedy(), tokenizer=ids)
    assert all(torch.equal(o, w) for o, w in zip(outs, want)), ([o.tolist() for o in outs], [w.tolist() for w in want])
    assert torch.equal(scores, want_scores)


def test_single_prompt_is_generate_on_device(golden_dir):
    z, c, ids, model = _golden(golden_dir)
    a = _prompts(z, c, 4)[0]
    outs, scores = generate_batch_on_device(model, [a.clone()], _sampled(), tokenizer=ids, seed=77)
    want, want_scores = generate_on_device(model, a.clone(), _sampled(), tokenizer=ids, seed=77)
    assert len(outs) == 1 and torch.equal(outs[0], want)
    assert scores.shape == (1, 4) and torch.equal(scores[0], want_scores)
