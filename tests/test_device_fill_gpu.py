"""GPU: given ids inside a captured decode run -- the sampler's given table (cogv_sample_desc.given through
ops.sample_logits), generation.DeviceFiller against filling_sequence, its own eager form and a fresh filler after reuse,
magnify (super-resolution) end to end on the device, and the 64 x 64 decode that ends super-resolution."""
import types

import pytest
import torch

from cogview_amd import ops
from cogview_amd.generation import DeviceFiller, filling_sequence, magnify, top_k_logits
from oracle import cogview_oracle as O
from tests.generation_cases import COIN_FLIP, ToyIds, build_model, load_golden

pytestmark = pytest.mark.gpu

MIDFIX = ("[EOI1]", "[ROI2]", "[POS0]", "[BASE]", "[BOI2]")


def _toy(golden_dir):
    """The golden's toy model with a key/value memory as long as the filler's capacity: filling_sequence must not drop
    the oldest positions of a 1300-position window (its decode graph keeps every one)."""
    z, c = load_golden(golden_dir)
    return z, c, ToyIds(c["img_tokens"], c["txt_tokens"]), build_model(z, dict(c, max_mem=1408), "cuda", True)


def _window(z, c, ids, lines=30, given_lines=18, seed=0):
    """A magnify-shaped window: the golden's text, a 16 x 16 patch, the marker run, then `lines` lines of 32 codes whose
    first 16 codes are given in the first `given_lines` lines (the left neighbour's columns)."""
    g = torch.Generator().manual_seed(seed)
    n_img = c["img_tokens"]
    text = z["t2i_seq"][:6].tolist()
    patch = torch.randint(0, n_img, (256,), generator=g).tolist()
    target = torch.full((lines, 32), -1, dtype=torch.long)
    target[:given_lines, :16] = torch.randint(0, n_img, (given_lines, 16), generator=g)
    return torch.tensor(text + patch + [ids[m] for m in MIDFIX] + target.reshape(-1).tolist(), device="cuda")


def _args(top_k=1, temperature=1.0):
    return types.SimpleNamespace(temperature=temperature, top_k=top_k, top_p=0.0, is_sparse=0)


def _teacher_forced_gaps(model, row, ids, n_img):
    """Full forward of a completed window (positions by filling_sequence's [ROI2] rule): for every position i, the argmax
    over the image codes of the logits that predict it, and its top-2 gap in units of those logits' std."""
    s = row.numel()
    offset = row.tolist().index(ids["[ROI2]"])
    pos = torch.arange(s, device=row.device)
    pos[pos > offset] -= offset
    mask = torch.tril(torch.ones((1, s, s), device=row.device)).unsqueeze(1)
    with torch.no_grad():
        logits, *_ = model(row.view(1, -1), pos.view(1, -1), mask, None, None, 0)
    x = logits[0, :-1, :n_img].float()
    top = torch.topk(x, 2, dim=-1)
    gap = (top[0][:, 0] - top[0][:, 1]) / x.std(dim=-1)
    pad = torch.full((1,), -1, dtype=torch.long, device=row.device)
    return torch.cat([pad, top[1][:, 0]]), torch.cat([pad.float(), gap])


def _check_generated_at_argmax(model, seq, out, ids, n_img):
    """Given ids come back exactly; every generated id is the teacher-forced argmax unless its top-2 gap is a coin flip."""
    given = seq >= 0
    assert torch.equal(out[given], seq[given])
    arg, gap = _teacher_forced_gaps(model, out, ids, n_img)
    gen = ~given
    bad = gen & (out != arg) & (gap >= COIN_FLIP)
    assert not bad.any(), [(int(i), float(gap[i])) for i in bad.nonzero().flatten()[:8]]


def test_sampler_feeds_a_given_id_and_draws_elsewhere():
    V, cap, rows = 8704, 16, 2
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(rows, V, generator=g) * 3).half().cuda()
    masked = ((torch.arange(cap) | (1 << 31)) - (1 << 32)).to(torch.int32)

    def state():
        return dict(tok=torch.zeros(rows, dtype=torch.long), pos=torch.tensor([40, 41]), pos_index=torch.tensor([5]),
                    table=masked.repeat(rows, 1), counter=torch.zeros(1, dtype=torch.int32),
                    out_tokens=torch.full((rows, cap), -7, dtype=torch.long), ids=torch.zeros(rows, dtype=torch.long),
                    logp=torch.full((rows,), 9.0), scores=torch.tensor([0.5, -1.0]), offset=torch.tensor([3]))

    def call(st, given):
        st = {k: v.cuda() for k, v in st.items()}
        dec = dict(tok=st["tok"], pos=st["pos"], pos_index=st["pos_index"], table=st["table"], counter=st["counter"],
                   out_tokens=st["out_tokens"], out_base=0, given=given)
        ops.sample_logits(logits, temperature=1.02, top_k=200, allow=(0, 8192), seed=11, offset=st["offset"], ids=st["ids"],
                          logp=st["logp"], scores=st["scores"], decode=dec)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in st.items()}

    given = torch.full((cap,), -1, dtype=torch.long)
    given[6] = 123
    given = given.cuda()
    s0 = state()
    s1 = call(s0, given)                                   # position 6 is given
    assert s1["ids"].tolist() == s1["tok"].tolist() == s1["out_tokens"][:, 6].tolist() == [123, 123]
    assert (s1["out_tokens"][:, torch.arange(cap) != 6] == -7).all()
    assert s1["logp"].tolist() == [0.0, 0.0]
    assert torch.equal(s1["scores"], s0["scores"])
    assert s1["pos"].tolist() == [41, 42] and int(s1["pos_index"]) == 6 and int(s1["offset"]) == 4
    want_table = masked.repeat(rows, 1)
    want_table[:, 6] = 6
    assert torch.equal(s1["table"], want_table) and int(s1["counter"]) == 0
    # position 7 is not given: bit-identical to the same call without a table
    a, b = call(s1, given), call(s1, None)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["pos_index"]) == 7 and int(a["offset"]) == 5 and (a["ids"] < 8192).all()
    assert torch.equal(a["out_tokens"][:, 7], a["ids"]) and (a["logp"] < 0).all()
    assert torch.allclose(a["scores"], s1["scores"] + a["logp"])
    with pytest.raises(ValueError):
        call(s1, given[:cap - 1])                          # shorter than the table


@pytest.mark.parametrize("capture", [True, False])
def test_greedy_fill_matches_filling_sequence(golden_dir, capture):
    z, c, ids, model = _toy(golden_dir)
    seq = _window(z, c, ids)
    out = DeviceFiller(model, _args(), capture=capture)(model, seq.clone(), _args(), tokenizer=ids)
    assert out.shape == (1, seq.numel()) and out.device == seq.device
    out = out[0]
    ref = filling_sequence(model, seq.clone(), _args(), tokenizer=ids)[0]
    given = seq >= 0
    assert torch.equal(out[given], seq[given]) and torch.equal(ref[given], seq[given])
    _, gap = _teacher_forced_gaps(model, out, ids, c["img_tokens"])
    diff = (out != ref).nonzero().flatten()
    if diff.numel():                                       # a first divergence only at a coin flip
        i = int(diff[0])
        assert gap[i] < COIN_FLIP, (i, float(gap[i]))
    assert int(out[~given].max()) < c["img_tokens"]


def test_captured_fill_equals_eager(golden_dir):
    z, c, ids, model = _toy(golden_dir)
    seq = _window(z, c, ids, seed=1)
    args = _args(top_k=200, temperature=1.02)
    res = []
    for cap in (True, False):
        f = DeviceFiller(model, args, seed=1234, capture=cap)
        res.append((f(model, seq.clone(), args, tokenizer=ids), f.scores))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    assert res[0][1].shape == (1,) and torch.isfinite(res[0][1]).all() and float(res[0][1]) < 0
    out, given = res[0][0][0], seq >= 0
    assert torch.equal(out[given], seq[given]) and int(out[~given].max()) < c["img_tokens"]
    # sampled, not greedy: the filter of filling_sequence keeps every drawn id (top-200 of the teacher-forced logits)
    s = out.numel()
    offset = out.tolist().index(ids["[ROI2]"])
    pos = torch.arange(s, device="cuda")
    pos[pos > offset] -= offset
    with torch.no_grad():
        logits, *_ = model(out.view(1, -1), pos.view(1, -1), torch.tril(torch.ones((1, s, s), device="cuda")).unsqueeze(1),
                           None, None, 0)
    gen = (~given).nonzero().flatten()
    x = logits[0, gen - 1, :c["img_tokens"]].float()
    top = torch.topk(x, 201, dim=-1)[0]
    edge = (top[:, 199] - top[:, 200]) / x.std(dim=-1)
    kept = torch.gather(top_k_logits(x.clone(), top_k=200), 1, out[gen].view(-1, 1)).squeeze(1) > -float("inf")
    assert (kept | (edge < COIN_FLIP)).all()


@pytest.mark.parametrize("form", ["fused", "op_by_op"])
def test_reused_filler_equals_a_fresh_one(golden_dir, monkeypatch, form):
    """A shorter window after a longer one through one filler gives what a fresh filler gives.  The fused decode step
    attends slots [0, pos] by count; the op-by-op composition (layers without Sandwich-LN) reads the visible slots from the
    decoder's index table, where the longer run's slots must not stay visible."""
    z, c, ids, model = _toy(golden_dir)
    if form == "op_by_op":
        from cogview_amd import functional
        monkeypatch.setattr(functional, "decode_chain_supported", lambda *a: False)
        for layer in model.module.transformer.layers:
            monkeypatch.setattr(layer, "scale_normalization", False)
    long_seq, short_seq = _window(z, c, ids, lines=32, given_lines=0, seed=2), _window(z, c, ids, lines=18, seed=3)
    reused = DeviceFiller(model, _args())
    reused(model, long_seq.clone(), _args(), tokenizer=ids)
    a = reused(model, short_seq.clone(), _args(), tokenizer=ids)
    b = DeviceFiller(model, _args())(model, short_seq.clone(), _args(), tokenizer=ids)
    assert torch.equal(a, b)


def test_filler_rearm(golden_dir):
    """a sampled window, then a greedy one through the same filler: other sampler values re-arm the sampler and capture again
    while a graph exists, and give what a fresh greedy filler gives (top_k = 1: the draws do not depend on the generator offset
    the re-arm keeps)"""
    z, c, ids, model = _toy(golden_dir)
    first, second = _window(z, c, ids, lines=2, given_lines=1, seed=5), _window(z, c, ids, lines=2, given_lines=1, seed=6)
    assert first.numel() == 331
    sampled = _args(top_k=200, temperature=1.02)
    reused = DeviceFiller(model, sampled, capacity=384)
    reused(model, first.clone(), sampled, tokenizer=ids)
    graph = reused.dec.graph
    assert graph is not None
    a = reused(model, second.clone(), _args(), tokenizer=ids)
    assert reused.dec.graph is not None and reused.dec.graph is not graph
    fresh = DeviceFiller(model, _args(), capacity=384)
    b = fresh(model, second.clone(), _args(), tokenizer=ids)
    assert torch.equal(a, b) and torch.equal(reused.scores, fresh.scores)


def test_magnify_on_the_device(golden_dir):
    z, c, ids, model = _toy(golden_dir)
    n_img = c["img_tokens"]
    g = torch.Generator().manual_seed(4)
    code = torch.randint(0, n_img, (1024,), generator=g).cuda()
    text = torch.from_numpy(z["t2i_seq"][:6]).cuda()
    filler = DeviceFiller(model, _args())
    windows = []

    def fill(model_, seq, args, invalid_slices=None, tokenizer=None):
        out = filler(model_, seq, args, invalid_slices=invalid_slices, tokenizer=tokenizer)
        windows.append((seq.clone(), out[0].clone()))
        return out

    big = magnify(model, ids, code, text, _args(), fill=fill)
    assert big.shape == (1, 4096) and int(big.min()) >= 0 and int(big.max()) < n_img
    assert len(windows) == 9 and sum(int((s >= 0).sum()) - 267 for s, _ in windows) == 2384 + 1952 + 16
    for seq, out in windows:
        _check_generated_at_argmax(model, seq, out, ids, n_img)
    # the assembled map holds what the window that last wrote each line returned
    from cogview_amd.generation.sampling import _MAGNIFY_WINDOWS
    want = torch.full((64, 64), -1, dtype=torch.long, device="cuda")
    for (bi, bj, lines), (_, out) in zip(_MAGNIFY_WINDOWS, windows):
        want[16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)] = out[267:].view(lines, 32)
    assert torch.equal(big.view(64, 64), want)


def test_code2img_of_a_64x64_map_vs_oracle():
    """super-resolution's last step: a 64 x 64 code map decodes to a 512 x 512 image."""
    from cogview_amd import vqvae
    torch.manual_seed(0)
    m = vqvae.new_model().eval()
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ids = torch.randint(0, 8192, (1, 4096), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = O.code2img_denorm(O.vqvae_decode(ids.view(1, 64, 64), p))
    out = vqvae.code2img(m.cuda(), ids.cuda())
    assert out.shape == (1, 3, 512, 512)
    rel = float((out.cpu().double() - want.double()).norm() / want.double().norm())
    assert rel < 1e-5, rel
