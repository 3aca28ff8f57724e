"""GPU: the token sampler (cogv_sample_logits through ops.sample_logits) against the host filter of generation/sampling.py,
its draws against the distribution it reports, and generation.generate_on_device (prefill + captured decode graph with the
sampler inside) against the reference's greedy golden, its own eager form, and a teacher-forced full forward."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cogview_amd import ops
from cogview_amd.generation import add_interlacing_beam_marks, generate_on_device, top_k_logits
from tests.generation_cases import COIN_FLIP, ToyIds, build_model, check_tokens, load_golden

pytestmark = pytest.mark.gpu

V = 58240


def _rows(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, V, generator=g) * 3.0
    x[0::2] = torch.round(x[0::2] * 4) / 4                 # coarse grid: many ties everywhere, the k-th value included
    x[1, 17], x[1, 40000] = x[1].max() + 1, x[1].max() + 1  # a tie at the top
    x[3, 5:9] = x[3].max() + 0.5                            # four-way tie at the top
    return x.to(dtype)


def _host_filter(x, T, k, p, lo, hi):
    """filling_sequence's filter in fp32 (sampling.py: /temperature, invalid slices, top_k_logits), top-p per row with
    ties kept together.  Returns (probs in fp64, mass strictly above each id in the top-k distribution)."""
    x = x.float() / T
    x[:, :lo] = -float("inf")
    x[:, hi:] = -float("inf")
    x = top_k_logits(x, top_k=k)
    above = torch.zeros_like(x)
    if p > 0:
        pk = F.softmax(x, dim=-1)
        for r in range(x.shape[0]):
            v, order = torch.sort(x[r], descending=True)
            excl = torch.cumsum(pk[r][order], 0) - pk[r][order]
            first = torch.ones_like(v, dtype=torch.bool)
            first[1:] = v[1:] != v[:-1]
            grp = torch.cumsum(first.long(), 0) - 1                  # tie group of each sorted position
            gmass = excl[first][grp]                                 # mass strictly above the group
            a = torch.empty_like(gmass)
            a[order] = gmass
            above[r] = a
            x[r][a > p] = -float("inf")
    # values in fp64 over the fp32 filter's kept set: torch's fp32 softmax is itself ~7e-6 (relative) off on 58 240 ids
    return F.softmax(x.double(), dim=-1), above


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_kept_set_and_probabilities_match_the_host_filter(dtype):
    x = _rows(dtype).cuda()
    xc = x.cpu()
    worst = 0.0
    for T in (1.0, 1.02, 0.7):
        for k in (0, 1, 5, 200, 8192):
            for p in (0.0, 0.5, 0.9):
                for lo, hi in ((0, V), (0, 8192)):
                    _, _, got = ops.sample_logits(x, temperature=T, top_k=k, top_p=p, allow=(lo, hi), seed=3, probs=True)
                    got = got.cpu()
                    want, above = _host_filter(xc, T, k, p, lo, hi)
                    diff = (got > 0) != (want > 0)
                    if p == 0:
                        assert not diff.any(), (T, k, p, lo, int(diff.sum()))
                    else:
                        assert ((above[diff] - p).abs() < 1e-6).all(), (T, k, p, lo, (above[diff] - p).abs().max())
                    both = (got > 0) & (want > 0)
                    rel = ((got[both] - want[both]).abs() / want[both]).max().item()
                    if not diff.any():
                        assert rel < 3e-6, (T, k, p, lo, rel)
                    worst = max(worst, rel)
    print(f"[{dtype}] worst relative probability error {worst:.2e}")


def test_draws_follow_the_reported_distribution():
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(1, V, generator=g) * 2.0).cuda()
    rows, offsets = 4096, 16                                       # 2^16 draws
    ids = []
    for off in range(offsets):
        i, lp, pr = ops.sample_logits(row, top_k=200, seed=11, offset=off, rows=rows, probs=True)
        ids.append(i.clone())
        probs = pr[0]
        assert torch.allclose(lp, torch.log(probs[i]), rtol=0, atol=1e-5)
    again, _, _ = ops.sample_logits(row, top_k=200, seed=11, offset=3, rows=rows)
    assert torch.equal(again, ids[3]), "same (seed, offset) must give the same ids"
    assert not torch.equal(ids[3], ids[4]), "consecutive offsets must give different streams"
    allids = torch.cat(ids).cpu()
    probs = probs.cpu().double()
    assert (probs[allids] > 0).all(), "an id outside the kept set was drawn"
    assert int((probs > 0).sum()) == 200
    n = allids.numel()
    counts = torch.bincount(allids, minlength=V).double()
    kept = probs > 0
    e, o = n * probs[kept], counts[kept]
    small = e < 5
    e = torch.cat([e[~small], e[small].sum().view(1)]) if small.any() else e
    o = torch.cat([o[~small], o[small].sum().view(1)]) if small.any() else o
    chi2 = float(((o - e) ** 2 / e).sum())
    dof = e.numel() - 1
    z = 4.753                                                       # upper 1e-6 quantile of the standard normal
    bound = dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3    # Wilson-Hilferty
    print(f"chi-square {chi2:.1f} with {dof} degrees of freedom (1e-6 bound {bound:.1f})")
    assert chi2 < bound


def _golden_model(golden_dir):
    z, c = load_golden(golden_dir)
    return z, c, ToyIds(c["img_tokens"], c["txt_tokens"]), build_model(z, c, "cuda", True)


@pytest.mark.parametrize("capture", [True, False])
def test_greedy_generation_reproduces_the_reference_golden(golden_dir, capture):
    z, c, ids, model = _golden_model(golden_dir)
    seq = torch.from_numpy(z["t2i_seq"]).cuda()
    add_interlacing_beam_marks(seq, nb=c["beams"])
    args = types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)
    out, scores = generate_on_device(model, seq.clone(), args, tokenizer=ids, capture=capture)
    check_tokens(out.cpu(), z, c)
    assert scores.shape == (c["beams"],) and torch.isfinite(scores).all()
    assert (scores.abs() < 1e-4).all()                              # greedy: log 1 per token


@pytest.mark.parametrize("nb", [1, 8])
def test_captured_generation_equals_eager(golden_dir, nb):
    z, c, ids, model = _golden_model(golden_dir)
    seq = torch.from_numpy(z["t2i_seq"]).cuda()
    add_interlacing_beam_marks(seq, nb=nb)
    args = types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)
    res = [generate_on_device(model, seq.clone(), args, tokenizer=ids, seed=1234, capture=cap) for cap in (True, False)]
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1])
    out = res[0][0]
    assert out.shape == (nb, seq.numel()) and int(out[:, 8:].max()) < c["img_tokens"]
    if nb > 1:
        assert len({tuple(r) for r in out[:, 8:].tolist()}) > 1, "independent rows drew identical sequences"


def test_teacher_forced_consistency(golden_dir):
    z, c, ids, model = _golden_model(golden_dir)
    seq = torch.from_numpy(z["t2i_seq"]).cuda()
    add_interlacing_beam_marks(seq, nb=2)
    n = int((seq >= 0).sum())
    args = types.SimpleNamespace(temperature=1.0, top_k=200, top_p=0.0, is_sparse=0)
    out, scores = generate_on_device(model, seq.clone(), args, tokenizer=ids, seed=7)
    pos = torch.arange(out.shape[1], device="cuda").unsqueeze(0).expand_as(out)
    with torch.no_grad():
        logits, *_ = model(out, pos, 0, None, None, 0)
    x = logits[:, n - 1:-1].float()
    x[..., c["img_tokens"]:] = -float("inf")
    std = x[..., :c["img_tokens"]].std(dim=-1)
    top = torch.topk(x, 201, dim=-1)[0]
    gap = (top[..., 199] - top[..., 200]) / std
    filt = top_k_logits(x.clone(), top_k=200)
    gen = out[:, n:]
    inside = torch.gather(filt, 2, gen.unsqueeze(-1)).squeeze(-1) > -float("inf")
    assert (inside | (gap < COIN_FLIP)).all(), (gap[~inside]).tolist()
    if inside.all():
        want = torch.gather(F.log_softmax(filt, dim=-1), 2, gen.unsqueeze(-1)).squeeze(-1).sum(-1)
        # the decode steps' fp16 logits differ from the full forward's by up to 3e-3 rel-L2 (the GraphDecoder test's bar): a
        # few 1e-4 per token in log-probability, summed over the run
        assert torch.allclose(scores, want, rtol=0, atol=2.5e-4 * gen.shape[1]), (scores.tolist(), want.tolist())


def test_unsupported_forms_raise(golden_dir):
    z, c, ids, model = _golden_model(golden_dir)
    seq = torch.from_numpy(z["t2i_seq"]).cuda()
    args = types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        generate_on_device(model, torch.cat([seq, seq[:1]]), args, tokenizer=ids)
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        generate_on_device(model, seq, types.SimpleNamespace(**{**vars(args), "is_sparse": 2}), tokenizer=ids)
    s = seq.clone()
    add_interlacing_beam_marks(s, nb=3, period=10)
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        generate_on_device(model, s, args, tokenizer=ids)
