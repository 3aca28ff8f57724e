"""GPU: super-resolution for several images on one decode graph -- the sampler's per-row given table (cogv_sample_desc.given_stride
through ops.sample_logits), generation.DeviceBatchFiller against each row's teacher-forced argmax, its own eager form, a fresh
filler after reuse, chunk steps, the 8-bit formats, nine rows, and magnify_batch end to end on the device.

Windows are those of tests/test_device_fill_gpu.py on the toy golden model, with the first 6 - n text ids dropped for a text of n
ids.  `_window(lines=2, given_lines=1)` (331 positions at 6 text ids) has its 16 given codes in line 0, where they join the
context; a window with given ids INSIDE the run -- what a table shared by all rows would get wrong -- needs a given line after a
generated one: lines=3, given_lines=2 (363 positions, 16 given ids inside the run).  Both shapes are used."""
import pytest
import torch

from cogview_amd import ops
from cogview_amd.generation import DeviceBatchFiller, magnify_batch, plan_chunk_steps, plan_device_batch_fill
from tests.generation_cases import COIN_FLIP, ToyIds
from tests.test_device_fill_gpu import MIDFIX, _args, _teacher_forced_gaps, _toy, _window

pytestmark = pytest.mark.gpu

_TOY = {}


def _golden(golden_dir):
    if not _TOY:
        _TOY["v"] = _toy(golden_dir)
    return _TOY["v"]


def _windows(z, c, ids, lengths=(6, 4, 2), lines=2, given_lines=1, seed=10):
    """one window per text length: other patches and other given ids in every row"""
    return [_window(z, c, ids, lines=lines, given_lines=given_lines, seed=seed + g)[6 - n:] for g, n in enumerate(lengths)]


def _check_rows(model, seqs, outs, ids, n_img, tally):
    """Per row: given ids come back exactly, every generated id is the row's teacher-forced argmax unless its top-2 gap is a coin
    flip.  tally += [generated ids off the argmax, generated ids]."""
    assert len(outs) == len(seqs)
    for g, (seq, out) in enumerate(zip(seqs, outs)):
        assert out.shape == (1, seq.numel()) and out.device == seq.device
        out = out[0]
        given = seq >= 0
        assert torch.equal(out[given], seq[given]), f"row {g}: given ids changed"
        arg, gap = _teacher_forced_gaps(model, out, ids, n_img)
        off = ~given & (out != arg)
        bad = off & (gap >= COIN_FLIP)
        assert not bad.any(), (g, [(int(i), float(gap[i])) for i in bad.nonzero().flatten()[:8]])
        tally[0] += int(off.sum())
        tally[1] += int((~given).sum())


def _within_budget(tally):
    """the coin-flip excuse cannot hide a failure: at most 5 % of the generated ids of a test may be off the argmax"""
    print(f"{tally[0]} of {tally[1]} generated ids off the teacher-forced argmax (all at top-2 gaps below {COIN_FLIP} std)")
    assert tally[0] <= 0.05 * tally[1], tally


# ------------------------------------------------------------------------------------------------------- 1. the sampler's table
def test_sampler_reads_a_given_table_per_row():
    V, cap, rows = 8704, 16, 3
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(rows, V, generator=g) * 3).half().cuda()
    masked = ((torch.arange(cap) | (1 << 31)) - (1 << 32)).to(torch.int32)

    def state():
        return dict(tok=torch.zeros(rows, dtype=torch.long), pos=torch.tensor([40, 41, 42]), pos_index=torch.tensor([5]),
                    table=masked.repeat(rows, 1), counter=torch.zeros(1, dtype=torch.int32),
                    out_tokens=torch.full((rows, cap), -7, dtype=torch.long), ids=torch.zeros(rows, dtype=torch.long),
                    logp=torch.full((rows,), 9.0), scores=torch.tensor([0.5, -1.0, 0.25]), offset=torch.tensor([3]))

    def call(st, given):
        st = {k: v.cuda() for k, v in st.items()}
        dec = dict(tok=st["tok"], pos=st["pos"], pos_index=st["pos_index"], table=st["table"], counter=st["counter"],
                   out_tokens=st["out_tokens"], out_base=0, given=given)
        ops.sample_logits(logits, temperature=1.02, top_k=200, allow=(0, 8192), seed=11, offset=st["offset"], ids=st["ids"],
                          logp=st["logp"], scores=st["scores"], decode=dec)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in st.items()}

    table = torch.full((rows, cap), -1, dtype=torch.long)
    table[:, 6] = torch.tensor([123, 4567, 8])              # (a) slot 6: every row its own id
    table[0, 7] = 77                                        # (b) slot 7: row 0 is fed, rows 1 and 2 draw
    given = table.cuda()
    s0 = state()
    s1 = call(s0, given)
    assert s1["ids"].tolist() == s1["tok"].tolist() == s1["out_tokens"][:, 6].tolist() == [123, 4567, 8]
    assert (s1["out_tokens"][:, torch.arange(cap) != 6] == -7).all()
    assert s1["logp"].tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(s1["scores"], s0["scores"])
    assert s1["pos"].tolist() == [41, 42, 43] and int(s1["pos_index"]) == 6 and int(s1["offset"]) == 4
    want_table = masked.repeat(rows, 1)
    want_table[:, 6] = 6
    assert torch.equal(s1["table"], want_table) and int(s1["counter"]) == 0
    a, b = call(s1, given), call(s1, None)
    assert int(a["ids"][0]) == int(a["tok"][0]) == int(a["out_tokens"][0, 7]) == 77
    assert float(a["logp"][0]) == 0.0 and float(a["scores"][0]) == float(s1["scores"][0])
    assert (b["logp"] < 0).all() and (b["ids"] < 8192).all()
    for k in ("ids", "tok", "logp", "scores", "out_tokens"):
        assert torch.equal(a[k][1:], b[k][1:]), k           # the rows that draw: the bits of a call without a table
    for k in ("pos", "pos_index", "offset", "counter", "table"):
        assert torch.equal(a[k], b[k]), k                   # the bookkeeping of a draw
    assert int(a["pos_index"]) == 7 and int(a["offset"]) == 5 and int(a["counter"]) == 0
    # (c) a 2-D table whose rows are all equal is the 1-D table; the row stride is the tensor's
    one = torch.full((cap,), -1, dtype=torch.long)
    one[6] = 123
    one = one.cuda()
    wide = one.repeat(rows, 2)                               # [rows, 2 * cap]: rows 2 * cap elements apart
    for st in (s0, s1):                                      # a given slot and a drawn one
        want = call(st, one)
        for got in (call(st, one.repeat(rows, 1)), call(st, wide), call(st, wide[:, :cap])):
            for k in want:
                assert torch.equal(got[k], want[k]), k
    # (d) a wrong row count, too few columns
    with pytest.raises(ValueError):
        call(s1, given[:2])
    with pytest.raises(ValueError):
        call(s1, given[:, :cap - 1].contiguous())
    with pytest.raises(ValueError):
        call(s1, given.to(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. a greedy batch of windows
@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("lines,given_lines", [(2, 1), (3, 2)], ids=["given_in_context", "given_inside_the_run"])
def test_greedy_batch_of_three_windows(golden_dir, capture, lines, given_lines):
    z, c, ids, model = _golden(golden_dir)
    seqs = _windows(z, c, ids, lines=lines, given_lines=given_lines)
    assert [s.numel() for s in seqs] == [267 + 32 * lines - d for d in (0, 2, 4)]
    plan = plan_device_batch_fill([s.tolist() for s in seqs], ids, int(z["vocab"]))
    assert plan["pads"] == [0, 2, 4] and sum(t >= 0 for t in plan["given"][1]) == 16 * (given_lines - 1)
    if given_lines > 1:                                      # every row carries its own ids at the same slots
        assert len({tuple(t for t in row if t >= 0) for row in plan["given"]}) == 3
    f = DeviceBatchFiller(model, _args(), rows=3, capacity=384, capture=capture)
    outs = f([s.clone() for s in seqs], tokenizer=ids)
    assert (f.dec.graph is not None) == capture and f.model_calls == plan["replays"]
    assert f.scores.shape == (3,) and f.scores.dtype == torch.float32
    tally = [0, 0]
    _check_rows(model, seqs, outs, ids, c["img_tokens"], tally)
    _within_budget(tally)


# ---------------------------------------------------------------------------------------------------- 3. captured equals eager
def _sampled():
    return _args(top_k=200, temperature=1.02)


def _captured_and_eager(model, seqs, ids, args, rows, capacity=384, **kw):
    res = []
    for cap in (True, False):
        f = DeviceBatchFiller(model, args, rows=rows, capacity=capacity, seed=1234, capture=cap, **kw)
        res.append((f([s.clone() for s in seqs], tokenizer=ids), f.scores, f))
    (outs, scores, f), (outs_e, scores_e, _) = res
    assert all(torch.equal(a, b) for a, b in zip(outs, outs_e)) and torch.equal(scores, scores_e)
    for seq, out in zip(seqs, outs):
        assert torch.equal(out[0][seq >= 0], seq[seq >= 0])
    return outs, scores, f


@pytest.mark.parametrize("lines,given_lines", [(2, 1), (3, 2)], ids=["given_in_context", "given_inside_the_run"])
def test_captured_batch_fill_equals_eager(golden_dir, lines, given_lines):
    z, c, ids, model = _golden(golden_dir)
    seqs = _windows(z, c, ids, lines=lines, given_lines=given_lines)
    outs, scores, _ = _captured_and_eager(model, seqs, ids, _sampled(), 3)
    assert scores.shape == (3,) and torch.isfinite(scores).all() and (scores < 0).all()
    for seq, out in zip(seqs, outs):
        assert int(out[0][seq < 0].min()) >= 0 and int(out[0][seq < 0].max()) < c["img_tokens"]


# ------------------------------------------------------------------------------------------------------------------- 4. reuse
def test_reused_batch_filler_equals_a_fresh_one(golden_dir):
    z, c, ids, model = _golden(golden_dir)
    long_set = _windows(z, c, ids, lines=4, given_lines=0, seed=20)
    short_set = _windows(z, c, ids, lines=2, given_lines=1, seed=30)
    reused = DeviceBatchFiller(model, _args(), rows=3, capacity=448)
    reused([s.clone() for s in long_set], tokenizer=ids)
    graph = reused.dec.graph
    a = reused([s.clone() for s in short_set], tokenizer=ids)
    assert reused.dec.graph is graph and graph is not None
    fresh = DeviceBatchFiller(model, _args(), rows=3, capacity=448)
    b = fresh([s.clone() for s in short_set], tokenizer=ids)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(reused.scores, fresh.scores)
    # two sequences through the filler of three rows: the spare row repeats the last one and is dropped
    two = _windows(z, c, ids, lengths=(3, 6), lines=3, given_lines=2, seed=40)
    outs = reused([s.clone() for s in two], tokenizer=ids)
    assert len(outs) == 2 and reused.scores.shape == (2,) and reused.dec.graph is graph
    tally = [0, 0]
    _check_rows(model, two, outs, ids, c["img_tokens"], tally)
    _within_budget(tally)


# ------------------------------------------------------------------------------------------------------------------- 5. chunk
@pytest.mark.parametrize("rows,chunk", [(2, 4), (4, 2)])
def test_batch_fill_in_chunks(golden_dir, rows, chunk):
    z, c, ids, model = _golden(golden_dir)
    seqs = _windows(z, c, ids, lengths=(6, 3, 5, 1)[:rows], lines=3, given_lines=2, seed=50)
    plan = plan_device_batch_fill([s.tolist() for s in seqs], ids, int(z["vocab"]))
    widths = plan_chunk_steps(plan["pattern"], plan["P"], plan["replays"], chunk)
    outs, scores, f = _captured_and_eager(model, seqs, ids, _args(), rows, chunk=chunk)
    assert f.model_calls == len(widths) < plan["replays"] and f.dec.chunk_steps == sum(1 for w in widths if w > 1) > 0
    assert f.dec.graph is not None and f.dec.graph_chunk is not None
    tally = [0, 0]
    _check_rows(model, seqs, outs, ids, c["img_tokens"], tally)
    _within_budget(tally)


# ----------------------------------------------------------------------------------------------------------------- 6. formats
def _h1024():
    """the two-layer h = 1024 model of tests/test_kv8_decode_gpu.py (192 positions): the fused chain, the 8-bit weight stream and
    the wide step need h % 512 == 0"""
    from tests.test_kv8_decode_gpu import _model
    from tests.test_w8_decode_gpu import N_IMG, N_TXT
    return _model(torch.float16), ToyIds(N_IMG, N_TXT), N_IMG, N_TXT


def _small_windows(ids, n_img, n_txt, lengths, seed=60):
    """window-shaped sequences of at most 56 ids: text, 8 patch codes, the marker run, four lines of 8 codes whose first 4 are given
    in lines 0 .. 2 (line 0's join the context; 8 given ids, each row's own, inside the run)"""
    out = []
    for g_, n in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + g_)
        text = (n_img + torch.randint(0, n_txt, (n,), generator=g)).tolist()
        patch = torch.randint(0, n_img, (8,), generator=g).tolist()
        target = torch.full((4, 8), -1, dtype=torch.long)
        target[:3, :4] = torch.randint(0, n_img, (3, 4), generator=g)
        out.append(torch.tensor(text + patch + [ids[m] for m in MIDFIX] + target.reshape(-1).tolist(), device="cuda"))
    return out


@pytest.mark.parametrize("formats", [dict(kv="e4m3"), dict(weights="e4m3"), dict(kv="e4m3", weights="e4m3")], ids=["kv8", "w8", "kv8+w8"])
def test_captured_batch_fill_equals_eager_in_8_bits(formats):
    model, ids, n_img, n_txt = _h1024()
    seqs = _small_windows(ids, n_img, n_txt, (9, 4))
    outs, scores, _ = _captured_and_eager(model, seqs, ids, _sampled(), 2, capacity=64, **formats)
    assert torch.isfinite(scores).all() and (scores < 0).all()
    for seq, out in zip(seqs, outs):
        assert int(out[0][seq < 0].max()) < n_img


# --------------------------------------------------------------------------------------------------------------- 7. nine rows
def test_nine_rows(golden_dir):
    z, c, ids, model = _golden(golden_dir)
    seqs = _windows(z, c, ids, lengths=(6, 5, 4, 3, 2, 1, 6, 4, 2), lines=3, given_lines=2, seed=70)
    f = DeviceBatchFiller(model, _args(), rows=9, capacity=384)
    outs = f([s.clone() for s in seqs], tokenizer=ids)
    assert f.scores.shape == (9,) and f.dec.graph is not None
    tally = [0, 0]
    _check_rows(model, seqs, outs, ids, c["img_tokens"], tally)
    _within_budget(tally)


def test_nine_rows_on_the_wide_step():
    """h = 1024: nine rows take the weight-streaming wide step; 8-bit weights stop at 8 rows"""
    from cogview_amd import functional as F_
    model, ids, n_img, n_txt = _h1024()
    assert F_.decode_wide_supported(model.module.transformer, 9)
    seqs = _small_windows(ids, n_img, n_txt, (9, 4, 7, 1, 3, 11, 2, 5, 8), seed=80)
    outs, scores, _ = _captured_and_eager(model, seqs, ids, _sampled(), 9, capacity=64)
    assert scores.shape == (9,) and torch.isfinite(scores).all()
    assert len({tuple(out[0][seq < 0].tolist()) for seq, out in zip(seqs, outs)}) == 9
    with pytest.raises(NotImplementedError, match="weights='e4m3'"):
        DeviceBatchFiller(model, _args(), rows=9, capacity=64, weights="e4m3")


# ------------------------------------------------------------------------------------------------------------ 8. magnify_batch
def test_magnify_batch_on_the_device(golden_dir):
    z, c, ids, model = _golden(golden_dir)
    n_img = c["img_tokens"]
    g = torch.Generator().manual_seed(4)
    codes = torch.randint(0, n_img, (2, 1024), generator=g).cuda()
    text = torch.from_numpy(z["t2i_seq"][:6]).cuda()
    texts = [text, text[3:]]
    filler = DeviceBatchFiller(model, _args(), rows=2)
    windows = []

    def fill(seqs, args, tokenizer=None):
        outs = filler(seqs, args, tokenizer=tokenizer)
        windows.append(([s.clone() for s in seqs], [o.clone() for o in outs]))
        return outs

    big = magnify_batch(model, ids, codes, texts, _args(), fill=fill)
    assert big.shape == (2, 4096) and int(big.min()) >= 0 and int(big.max()) < n_img
    assert len(windows) == 9
    tally = [0, 0]
    for seqs, outs in windows:
        assert len(seqs) == 2 and seqs[0].numel() - seqs[1].numel() == 3
        _check_rows(model, seqs, outs, ids, n_img, tally)
    _within_budget(tally)
    assert tally[1] == 2 * 4096
    # the assembled maps hold what the window that last wrote each line returned
    from cogview_amd.generation.sampling import _MAGNIFY_WINDOWS
    for g_, n_ctx in enumerate((267, 264)):
        want = torch.full((64, 64), -1, dtype=torch.long, device="cuda")
        for (bi, bj, lines), (_, outs) in zip(_MAGNIFY_WINDOWS, windows):
            want[16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)] = outs[g_][0, n_ctx:].view(lines, 32)
        assert torch.equal(big[g_].view(64, 64), want)
    assert not torch.equal(big[0], big[1])
