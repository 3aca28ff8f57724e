"""Text -> image generation latency of the 4B model (random weights, bf16): generation.generate_on_device (prefill +
captured decode graph with the sampler inside) against filling_sequence with the in-place key/value cache (kv_cache=True:
one eager model call and host sampling per token), for one 1024-code image at batch 1 and 8 (top_k 200, as the reference's
scripts/text2image.sh).  `--sampler-only`: just the sampler kernel, 8 rows of 58 240 bf16 logits (for a rocprofv3 kernel
trace of its own).  `--super-resolution`: one generation.magnify of a random 32 x 32 code map (nine windows, top_k 200,
temperature 1.02, as the reference's scripts/super_resolution.sh) with fill=DeviceFiller and with filling_sequence
(kv_cache=True), wall seconds per image for each and the split of the device form's decode replays.  `--post-selection`: the
reference's three stages joined on the device -- eight candidates from generate_on_device, scored with inverse_prompt_score
(the host tail: full logits in fp32) and with inverse_prompt_score_on_device in the same run (ms per candidate, largest score
difference, peak allocated memory of each), ranked by rerank_generated, the best one magnified with fill=DeviceFiller.
`--weights e4m3` (text -> image and `--super-resolution` legs): the device forms also run with the decode steps on 8-bit copies
of the weights (generate_on_device / DeviceFiller `weights=`), timed next to the 16-bit ones.  `--kv e4m3`: the same legs with the
8-bit key/value cache (`kv=`), alone or together with `--weights`.  `--chunk C` (`--super-resolution` leg): the same image again in
the same process with DeviceFiller(chunk=C) -- runs of given ids fed as chunk steps of C tokens -- next to the chunk=0 leg above:
seconds per image, model calls, and ms per replay of the one-token and of the chunk graph.  With `--kv e4m3` the chunk leg runs
once more on the 8-bit cache (DeviceFiller(chunk=C, kv="e4m3", kv_chunk=True), the opt-in).
`--super-resolution --images 1,4,8,16` (alone: no other leg runs): G images of different text lengths on ONE decode graph
(magnify_batch with DeviceBatchFiller(rows=G)), also rows=2 chunk=4 and rows=4 chunk=2, against images one after another
(magnify with DeviceFiller, chunk=0 and chunk=8, timed at the start and at the end of the process); seconds per image for each.
`--prompts G [--nb N]` (comma lists run several settings in one process: `--prompts 8,2 --nb 1,4`): G prompts of different text
lengths x N candidates each (default 1) for one 1024-code image per row, on ONE decode graph (generate_batch_on_device) against
the same prompts through generate_on_device one after another, in the same process; ms per generated token per prompt for each.
MB_GENERATE_SKIP_HOST=1 leaves out the filling_sequence legs (a parent-against-head comparison of the device forms)."""
import os, sys, time, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

if "--sampler-only" in sys.argv:
    from cogview_amd import ops
    x = torch.randn(8, 1, 58240, device="cuda").to(torch.bfloat16)
    ids = torch.empty(8, dtype=torch.int64, device="cuda")
    lp = torch.empty(8, dtype=torch.float32, device="cuda")
    for top_p in (0.0, 0.9):
        for i in range(50):
            ops.sample_logits(x, temperature=1.0, top_k=200, top_p=top_p, allow=(0, 8192), seed=1, offset=i, ids=ids, logp=lp)
    torch.cuda.synchronize()
    print("sampler: 2 x 50 launches of 8 rows x 58240 (top_k 200, top_p 0 / 0.9)")
    sys.exit(0)

os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29591")
import torch.distributed as dist
dist.init_process_group("nccl", init_method="env://", world_size=1, rank=0)
from cogview_amd import mpu
from cogview_amd.fp16 import FP16_Module
from cogview_amd.generation import (DeviceBatchFiller, DeviceFiller, IdSpace, magnify_batch, add_interlacing_beam_marks, filling_sequence, generate_batch_on_device,
                                    generate_on_device,
                                    inverse_prompt_score, inverse_prompt_score_on_device, magnify, plan_device_fill,
                                    post_selection_rows, rerank_generated)
from cogview_amd.model import GPT2Model
mpu.initialize_model_parallel(1); torch.manual_seed(1); mpu.model_parallel_cuda_manual_seed(1)
L, h, heads, V = 48, 2560, 40, 58240
SR = "--super-resolution" in sys.argv
SKIP_HOST = os.environ.get("MB_GENERATE_SKIP_HOST") == "1"
W8 = sys.argv[sys.argv.index("--weights") + 1] if "--weights" in sys.argv else None
KV8 = sys.argv[sys.argv.index("--kv") + 1] if "--kv" in sys.argv else None
CHUNK = int(sys.argv[sys.argv.index("--chunk") + 1]) if "--chunk" in sys.argv else 0
ids = IdSpace()
# super-resolution windows reach 1305 positions: filling_sequence's memory must hold them all, as the decode graph does
max_mem = 1408 if SR else 1089
model = FP16_Module(GPT2Model(L, V, h, heads, 0.1, 0.1, 0.1, 1089, max_mem, False, kv_cache=True).cuda(),
                    dtype=torch.bfloat16, keep_half_outputs=True).eval()
text = torch.randint(8192, 58192, (20,)).tolist()

if SR:
    args = types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.0, is_sparse=0)
    code = torch.randint(0, 8192, (1024,), device="cuda")
    text_t = torch.tensor(text, device="cuda")
    if "--images" in sys.argv:
        # several images per decode graph (magnify_batch + DeviceBatchFiller) against one image after another (magnify +
        # DeviceFiller), all in this process.  Every filler is warmed on the first window of its first image (prefill, capture of
        # its graphs, first-use allocations) and then timed over whole images; the one-image fillers are timed over one image each
        # at the start AND at the end of the process (their per-image time does not depend on how many images follow; the two
        # readings show the drift inside the process).
        Gs = [int(x) for x in sys.argv[sys.argv.index("--images") + 1].split(",")]
        gen = torch.Generator().manual_seed(7)
        midfix = torch.tensor([ids[m] for m in ("[EOI1]", "[ROI2]", "[POS0]", "[BASE]", "[BOI2]")], device="cuda")

        def images(G):                                                         # text lengths 20, 18, 23, 21, 26, ...
            codes = torch.randint(0, 8192, (G, 1024), generator=gen).cuda()
            return codes, [torch.randint(8192, 58192, (20 + 3 * (g // 2) - 2 * (g % 2),), generator=gen).cuda() for g in range(G)]

        def first_window(code, txt):
            return torch.cat([txt, code.view(32, 32)[:16, :16].reshape(-1), midfix, torch.full((18 * 32,), -1, dtype=torch.long, device="cuda")])

        def timed(fn):
            torch.cuda.synchronize(); t0 = time.time()
            out = fn()
            torch.cuda.synchronize()
            return out, time.time() - t0

        def one_after_another(chunk, n_images, tag):
            f = DeviceFiller(model, args, seed=1, chunk=chunk)
            codes, texts = images(n_images)
            f(model, first_window(codes[0], texts[0]), args, tokenizer=ids)                   # warm-up
            calls = []

            def fill(model_, seq, args_, invalid_slices=None, tokenizer=None):
                out = f(model_, seq, args_, invalid_slices, tokenizer)
                calls.append(f.model_calls)
                return out

            big, t = timed(lambda: [magnify(model, ids, c_, t_, args, fill=fill) for c_, t_ in zip(codes, texts)])
            assert all(b.shape == (1, 4096) and int(b.min()) >= 0 and int(b.max()) < 8192 for b in big)
            print(f"images one after another ({tag}): DeviceFiller chunk={chunk}, {n_images} image(s): {t / n_images:.2f} s per image, "
                  f"{sum(calls) // n_images} decode calls per image, {t / (sum(calls) + 9 * n_images) * 1e3:.2f} ms per model call", flush=True)
            del f
            torch.cuda.empty_cache()
            return t / n_images

        def batched(G, chunk=0):
            f = DeviceBatchFiller(model, args, rows=G, seed=1, chunk=chunk)
            codes, texts = images(G)
            f([first_window(c_, t_) for c_, t_ in zip(codes, texts)], tokenizer=ids)         # warm-up
            calls = []

            def fill(seqs_, args_, tokenizer=None):
                out = f(seqs_, args_, tokenizer=tokenizer)
                calls.append(f.model_calls)
                return out

            big, t = timed(lambda: magnify_batch(model, ids, codes, texts, args, fill=fill))
            assert big.shape == (G, 4096) and int(big.min()) >= 0 and int(big.max()) < 8192 and torch.isfinite(f.scores).all()
            assert G == 1 or len({tuple(b.tolist()) for b in big}) == G
            print(f"images on one decode graph: DeviceBatchFiller rows={G} chunk={chunk}: {t:.2f} s for {G} image(s) = {t / G:.2f} s per image, "
                  f"{sum(calls)} decode calls, {t / (sum(calls) + 9) * 1e3:.2f} ms per model call", flush=True)
            del f
            torch.cuda.empty_cache()
            return t / G

        base = {c_: [one_after_another(c_, 1, "start")] for c_ in (0, 8)}
        per_image = {(G, 0): batched(G) for G in Gs}
        for G, c_ in ((2, 4), (4, 2)):
            per_image[(G, c_)] = batched(G, c_)
        for c_ in (0, 8):
            base[c_].append(one_after_another(c_, 1, "end"))
        best = min(per_image, key=per_image.get)
        print("seconds per image: " + ", ".join(f"rows={G}{f' chunk={c_}' if c_ else ''} {t:.2f}" for (G, c_), t in per_image.items())
              + f"; one after another chunk=0 {base[0][0]:.2f} / {base[0][1]:.2f}, chunk=8 {base[8][0]:.2f} / {base[8][1]:.2f} (start / end); "
              f"best rows={best[0]} chunk={best[1]}: {min(base[8]) / per_image[best]:.2f}x the chunk=8 filler", flush=True)
        sys.exit(0)
    seqs = []
    filler = DeviceFiller(model, args, seed=1)

    def fill(model_, seq, args_, invalid_slices=None, tokenizer=None):
        seqs.append(seq.tolist())
        return filler(model_, seq, args_, invalid_slices, tokenizer)

    torch.cuda.synchronize(); t0 = time.time()
    big_dev = magnify(model, ids, code, text_t, args, fill=fill)
    torch.cuda.synchronize(); t_dev = time.time() - t0
    torch.cuda.synchronize(); t0 = time.time()
    big_host = big_dev if SKIP_HOST else magnify(model, ids, code, text_t, args)
    torch.cuda.synchronize(); t_host = float("nan") if SKIP_HOST else time.time() - t0
    assert big_dev.shape == big_host.shape == (1, 4096) and int(big_dev.max()) < 8192 and int(big_host.max()) < 8192
    plans = [plan_device_fill(s, ids, V) for s in seqs]
    replays = sum(p["replays"] for p in plans)
    given = sum(sum(1 for g in p["given"] if g >= 0) for p in plans)
    print(f"super-resolution, one image (9 windows, {sum(len(s) for s in seqs)} positions): DeviceFiller {t_dev:.2f} s "
          f"(prefills + capture included); filling_sequence kv_cache=True {t_host:.2f} s; speed-up {t_host / t_dev:.2f}x")
    print(f"device form: {len(plans)} prefills (each draws one code), {replays} decode replays = {replays - given} generated "
          f"+ {given} given inside the runs; {sum(p['trailing'] for p in plans)} trailing given ids copied on the host; "
          f"{t_dev / (replays + len(plans)) * 1e3:.2f} ms per model call", flush=True)
    if W8 or KV8:
        filler8 = DeviceFiller(model, args, seed=1, weights=W8, kv=KV8)
        torch.cuda.synchronize(); t0 = time.time()
        big8 = magnify(model, ids, code, text_t, args, fill=filler8)
        torch.cuda.synchronize(); t_w8 = time.time() - t0
        assert big8.shape == (1, 4096) and int(big8.max()) < 8192
        print(f"DeviceFiller weights={W8} kv={KV8}: {t_w8:.2f} s (quantization + prefills + capture included), "
              f"{t_w8 / (replays + len(plans)) * 1e3:.2f} ms per model call; {t_dev / t_w8:.2f}x the 16-bit device form", flush=True)
    def chunk_leg(**formats):
        """the same image with DeviceFiller(chunk=CHUNK, **formats): seconds, model calls, ms per replay of both graphs"""
        filler_c = DeviceFiller(model, args, seed=1, chunk=CHUNK, **formats)
        calls = []

        def fill_c(model_, seq, args_, invalid_slices=None, tokenizer=None):
            out = filler_c(model_, seq, args_, invalid_slices, tokenizer)
            calls.append(filler_c.model_calls)
            return out

        torch.cuda.synchronize(); t0 = time.time()
        big_c = magnify(model, ids, code, text_t, args, fill=fill_c)
        torch.cuda.synchronize(); t_c = time.time() - t0
        assert big_c.shape == (1, 4096) and int(big_c.max()) < 8192
        dec = filler_c.dec

        def replay_ms(graph, n=20):
            dec.pos_index.fill_(1000)                   # replays scribble on slots past every window's run; none past the capacity
            torch.cuda.synchronize(); t0 = time.time()
            for _ in range(n):
                graph.replay()
            torch.cuda.synchronize()
            return (time.time() - t0) / n * 1e3

        what = "".join(f" {k}={v}" for k, v in formats.items())
        cache = dec.kv8.tensors() if dec.kv8 is not None else dec.caches
        print(f"DeviceFiller chunk={CHUNK}{what}: {t_c:.2f} s per image (prefills + capture of both graphs included) against "
              f"{t_dev:.2f} s with chunk=0 in this process ({t_dev / t_c:.3f}x); {sum(calls)} decode calls of which {dec.chunk_steps} "
              f"chunk steps, against {replays}; one-token replay {replay_ms(dec.graph):.2f} ms, chunk replay "
              f"{replay_ms(dec.graph_chunk):.2f} ms; resident cache {sum(t.numel() * t.element_size() for t in cache) / 2 ** 30:.3f} GiB", flush=True)
        return t_c

    if CHUNK:
        t_c16 = chunk_leg()
        if KV8:
            # the chunk steps on the 8-bit cache (opt-in: kv_chunk=True), in the same process as the 16-bit chunk leg above
            t_c8 = chunk_leg(**({"weights": W8} if W8 else {}), kv=KV8, kv_chunk=True)
            print(f"chunk={CHUNK} on the 8-bit cache: {t_c16 / t_c8:.3f}x the 16-bit cache's chunk={CHUNK} filler", flush=True)
    sys.exit(0)
args = types.SimpleNamespace(temperature=1.0, top_k=200, top_p=0.0, is_sparse=0)

if "--post-selection" in sys.argv:
    nb, reps = 8, 3
    seq = [ids["[ROI1]"]] + text + [ids["[BASE]"], ids["[BOI1]"]] + [-1] * 1024
    add_interlacing_beam_marks(seq, nb=nb, period=3000)
    out, _ = generate_on_device(model, torch.tensor(seq, device="cuda"), args, seed=1)
    rows = post_selection_rows(out, ids)

    def measure(fn):
        fn()                                                                   # warm-up (first-use allocations)
        torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
        t0 = time.time()
        for _ in range(reps):
            scores = fn()
        torch.cuda.synchronize()
        return scores, (time.time() - t0) / reps / nb * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    s_host, ms_host, mb_host = measure(lambda: inverse_prompt_score(model, rows, args))
    s_dev, ms_dev, mb_dev = measure(lambda: inverse_prompt_score_on_device(model, rows, args))
    print(f"post-selection, {nb} candidates of {rows.shape[1]} ids ({rows.shape[1] - 1028} scored text positions): "
          f"inverse_prompt_score {ms_host:.2f} ms/candidate, peak {mb_host:.0f} MiB above the model; "
          f"inverse_prompt_score_on_device {ms_dev:.2f} ms/candidate, peak {mb_dev:.0f} MiB; "
          f"largest |score difference| {(s_host - s_dev).abs().max().item():.3e} (scores {s_dev.min().item():.2f} .. {s_dev.max().item():.2f})")
    best, sc, order = rerank_generated(model, out, args, keep=1)
    n = best.shape[1] - 1024
    sr_args = types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.0, is_sparse=0)
    torch.cuda.synchronize(); t0 = time.time()
    big = magnify(model, ids, best[0, -1024:], best[0, 1:n - 2], sr_args, fill=DeviceFiller(model, sr_args, seed=1))
    torch.cuda.synchronize()
    assert big.shape == (1, 4096) and int(big.max()) < 8192 and int(order[0]) == int(s_dev.argmax())
    print(f"generate_on_device -> rerank_generated (kept candidate {int(order[0])}, score {sc[0].item():.2f}) -> magnify with "
          f"DeviceFiller: {time.time() - t0:.2f} s for the 64 x 64 codes", flush=True)
    sys.exit(0)

if "--prompts" in sys.argv:
    Gs = [int(x) for x in sys.argv[sys.argv.index("--prompts") + 1].split(",")]
    nbs = [int(x) for x in sys.argv[sys.argv.index("--nb") + 1].split(",")] if "--nb" in sys.argv else [1] * len(Gs)
    assert len(Gs) == len(nbs)
    for G, nb in zip(Gs, nbs):
        seqs = []
        for g in range(G):                                                     # 20, 18, 23, 21, 26, ... text pieces
            t = torch.randint(8192, 58192, (20 + 3 * (g // 2) - 2 * (g % 2),)).tolist()
            seq = t + [ids["[BASE]"], ids["[BOI1]"]] + [-1] * 1024
            add_interlacing_beam_marks(seq, nb=nb, period=3000)
            seqs.append(torch.tensor(seq, device="cuda"))
        generate_batch_on_device(model, seqs, args, seed=0, weights=W8, kv=KV8)           # warm-up (first-use allocations)
        torch.cuda.synchronize(); t0 = time.time()
        outs, scores = generate_batch_on_device(model, seqs, args, seed=1, weights=W8, kv=KV8)
        torch.cuda.synchronize(); t_batch = time.time() - t0
        assert all(int(o[:, -1024:].max()) < 8192 and o.shape == (nb, len(s)) for o, s in zip(outs, seqs)) and torch.isfinite(scores).all()
        generate_on_device(model, seqs[0], args, seed=0, weights=W8, kv=KV8)              # warm-up
        torch.cuda.synchronize(); t0 = time.time()
        for seq in seqs:
            out, sc = generate_on_device(model, seq, args, seed=1, weights=W8, kv=KV8)
            assert int(out[:, -1024:].max()) < 8192 and torch.isfinite(sc).all()
        torch.cuda.synchronize(); t_seq = time.time() - t0
        print(f"{G} prompts x {nb} (contexts {[int((s >= 0).sum()) for s in seqs]}, weights={W8} kv={KV8}): one decode graph "
              f"{t_batch:.2f} s = {t_batch / 1024 / G * 1e3:.2f} ms per generated token per prompt; one after another {t_seq:.2f} s = "
              f"{t_seq / 1024 / G * 1e3:.2f} ms per generated token per prompt (prefill + capture included in both); "
              f"{t_seq / t_batch:.2f}x", flush=True)
    sys.exit(0)

# (`--nb 16,32,64` without `--prompts`: this leg at those row counts -- above 8 rows the decode graph holds the wide step)
for nb in ([int(x) for x in sys.argv[sys.argv.index("--nb") + 1].split(",")] if "--nb" in sys.argv else (1, 8)):
    seq = text + [ids["[BASE]"], ids["[BOI1]"]] + [-1] * 1024
    add_interlacing_beam_marks(seq, nb=nb, period=3000)
    seq = torch.tensor(seq, device="cuda")
    generate_on_device(model, seq.clone(), args, seed=0)                       # warm-up (first-use allocations)
    torch.cuda.synchronize(); t0 = time.time()
    out, scores = generate_on_device(model, seq.clone(), args, seed=1)
    torch.cuda.synchronize(); t_dev = time.time() - t0
    assert int(out[:, -1024:].max()) < 8192 and torch.isfinite(scores).all()
    torch.cuda.synchronize(); t0 = time.time()
    ref = out if SKIP_HOST else filling_sequence(model, seq.clone(), args)
    torch.cuda.synchronize(); t_host = float("nan") if SKIP_HOST else time.time() - t0
    assert ref.shape == out.shape
    print(f"batch {nb}: generate_on_device {t_dev:.2f} s = {t_dev / 1024 * 1e3:.2f} ms/token = {t_dev / nb:.3f} s per image (prefill + capture included); "
          f"filling_sequence kv_cache=True {t_host:.2f} s = {t_host / 1024 * 1e3:.2f} ms/token; speed-up {t_host / t_dev:.1f}x",
          flush=True)
    if W8 or KV8:
        generate_on_device(model, seq.clone(), args, seed=0, weights=W8, kv=KV8)         # warm-up
        torch.cuda.synchronize(); t0 = time.time()
        out8, scores8 = generate_on_device(model, seq.clone(), args, seed=1, weights=W8, kv=KV8)
        torch.cuda.synchronize(); t_w8 = time.time() - t0
        assert int(out8[:, -1024:].max()) < 8192 and torch.isfinite(scores8).all()
        print(f"batch {nb}: generate_on_device weights={W8} kv={KV8} {t_w8:.2f} s = {t_w8 / 1024 * 1e3:.2f} ms/token (quantization + prefill + "
              f"capture included); {t_dev / t_w8:.2f}x the 16-bit device form", flush=True)
