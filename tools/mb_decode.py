"""Single-token decode latency of the 4B model with a 1024-position memory: the captured HIP-graph decode step
(generation.GraphDecoder), eager K/V-cache memories (kv_cache=True) and the reference-style layer-input memories (every
step re-projects K and V of the whole memory).  `--weights e4m3` | `--weights mxfp4`: in the same run, the captured step on the 8-bit
or 4-bit copies of the weights (GraphDecoder(weights=...)) next to the 16-bit one -- ms per token of each, and the relative L2 / largest difference
of their logits on the step that was timed.  `--kv e4m3`: the same comparison for the 8-bit key/value cache
(GraphDecoder(kv="e4m3")) against the 16-bit cache, both on the weights `--weights` names (default: 16-bit).  MB_DECODE_SKIP_EAGER=1
skips the eager timing of the first decoder.  MB_DECODE_BATCH=b: b rows (up to 64).  From 9 rows on, three captured steps are timed
in turn in this process, on the cache `--kv` names: the wide step (ops.gemm_rows), the step with the switch off (what
COGV_DECODE_WIDE=0 runs: the tile kernels) and the 8-row step -- ms per step and per row of each, and the relative L2 / largest
difference of the first two's logits on the timed step.  With `--weights F` a fourth step joins that alternation: the captured step
on the quantized copies through the wide products (GraphDecoder(weights=F, wide=True)) -- its ms per step against the 16-bit wide
step and the switch-off step of the same process, and its logits' difference from the 16-bit wide step's.  (The 8-row comparison
of `--weights` below is for up to 8 rows and is skipped then.)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29589")
import torch, torch.distributed as dist
dist.init_process_group("nccl", init_method="env://", world_size=1, rank=0)
from cogview_amd import mpu
from cogview_amd.fp16 import FP16_Module
from cogview_amd.model import GPT2Model
mpu.initialize_model_parallel(1); torch.manual_seed(1); mpu.model_parallel_cuda_manual_seed(1)
L, h, heads, V = 48, 2560, 40, 58240
pre, steps = 1024, 24
tokens = torch.randint(0, 58219, (1, pre + steps), device="cuda")
pos = torch.arange(pre + steps, device="cuda").unsqueeze(0)
from cogview_amd.generation import GraphDecoder
model = FP16_Module(GPT2Model(L, V, h, heads, 0.1, 0.1, 0.1, 1089, 1089, False).cuda(), dtype=torch.bfloat16, keep_half_outputs=True).eval()
B = int(os.environ.get("MB_DECODE_BATCH", "1"))
if B >= 9:       # the wide step is measured at every row count its kernel takes, not only where the decoder takes it by default
    from cogview_amd import functional as F_
    F_._DECODE_WIDE_MAX_ROWS = F_.DECODE_WIDE_KERNEL_ROWS
tokens, pos = tokens.expand(B, -1).contiguous(), pos.expand(B, -1).contiguous()
dec = GraphDecoder(model, batch=B, capacity=1152)
with torch.no_grad():
    dec.prefill(tokens[:, :pre], pos[:, :pre])
    for mode in (("captured graph",) if os.environ.get("MB_DECODE_SKIP_EAGER") == "1" else ("eager fixed-capacity step", "captured graph")):
        if mode == "captured graph":
            dec.capture()
        for t in range(4):
            dec.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
        torch.cuda.synchronize(); t0 = time.time()
        for t in range(20):
            lg = dec.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
            nxt = lg[:, -1].float().argmax(-1)                   # consume the logits on the device, as a sampler would
        torch.cuda.synchronize(); dt = (time.time() - t0) / 20
        print(f"GraphDecoder {mode}: decode {dt*1e3:.2f} ms/token at memory length ~{pre}" + (f" (batch {B})" if B > 1 else ""), flush=True)
WFMT = sys.argv[sys.argv.index("--weights") + 1] if "--weights" in sys.argv else None
KVFMT = sys.argv[sys.argv.index("--kv") + 1] if "--kv" in sys.argv else None


def _alternate(base, other, base_name, other_name):
    """Both captured decoders at the same history, timed in turn, twice (the order must not matter).  Returns (ms, last logits)."""
    while other.length < base.length:
        other.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
    ms, last = {}, {}
    for rep in range(2):
        for name, d in ((base_name, base), (other_name, other)):
            d.length -= 24
            for t in range(4):
                d.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
            torch.cuda.synchronize(); t0 = time.time()
            for t in range(20):
                lg = d.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
                nxt = lg[:, -1].float().argmax(-1)
            torch.cuda.synchronize()
            ms.setdefault(name, []).append((time.time() - t0) / 20 * 1e3)
            last[name] = lg.float().clone()
    return ms, last


def _report(ms, last, a, b, what, tail=""):
    print(f"captured graph, {a}: {min(ms[a]):.2f} ms/token; {b}: {min(ms[b]):.2f} ms/token "
          f"({min(ms[a]) / min(ms[b]):.2f}x; runs {['%.2f' % v for v in ms[a]]} / {['%.2f' % v for v in ms[b]]})"
          + (f" (batch {B})" if B > 1 else "") + tail, flush=True)
    lg16, lg8 = last[a], last[b]
    print(f"logits {what} on the timed step: rel-L2 {((lg8 - lg16).norm() / lg16.norm()).item():.3e}, "
          f"max |difference| {(lg8 - lg16).abs().max().item():.3e} (max |logit| {lg16.abs().max().item():.3f})", flush=True)


def _captured(d, wide):
    """the prefilled decoder d captured and brought to the first decoder's history; wide=False: captured with
    functional._DECODE_WIDE off, i.e. the step a process started under COGV_DECODE_WIDE=0 runs (above 8 rows: the tile kernels of
    ops.gemm)"""
    from cogview_amd import functional as F_
    saved = F_._DECODE_WIDE
    F_._DECODE_WIDE = bool(wide) and saved
    try:
        with torch.no_grad():
            d.capture()
            for t in range(dec.length - d.length):
                d.step(tokens[:d.batch, pre:pre + 1], pos[:d.batch, pre:pre + 1])
    finally:
        F_._DECODE_WIDE = saved
    return d


def _prefilled(batch, kv, **more):
    d = GraphDecoder(model, batch=batch, capacity=1152, kv=kv, **more)
    with torch.no_grad():
        d.prefill(tokens[:batch, :pre], pos[:batch, :pre])
    return d


def _time_legs(legs):
    """the captured decoders of `legs` (name -> decoder), timed in turn, twice.  Returns (ms per step, last logits) by name."""
    ms, last = {}, {}
    for rep in range(2):
        for name, d in legs.items():
            tk, ps = tokens[:d.batch, pre:pre + 1], pos[:d.batch, pre:pre + 1]
            d.length -= 24
            for t in range(4):
                d.step(tk, ps)
            torch.cuda.synchronize(); t0 = time.time()
            for t in range(20):
                lg = d.step(tk, ps)
                nxt = lg[:, -1].float().argmax(-1)
            torch.cuda.synchronize()
            ms.setdefault(name, []).append((time.time() - t0) / 20 * 1e3)
            last[name] = lg.float().clone()
    return ms, last


if B >= 9:
    # the wide step (9 .. 64 rows: the five products of a layer as weight streams, ops.gemm_rows) against the step with the switch
    # off and against the 8-row step, all captured, in this process; on the cache format --kv names
    from cogview_amd import functional as F_
    wide_on = F_.decode_wide_supported(model.module.transformer, B)
    # Every prefill BEFORE the captures: above 8 rows the switched-off step runs split-K tile kernels, whose shared workspace
    # (ops.workspace, regrown on demand) is baked into its graph -- a later prefill that needs a larger one (8 x 1024 rows: 252 MB
    # for the 4h -> h product) would replace the buffer under the captured graph.
    made = [_prefilled(B, KVFMT) if KVFMT is not None else dec, _prefilled(B, KVFMT), _prefilled(8, KVFMT)]
    if WFMT is not None:
        made.append(_prefilled(B, KVFMT, weights=WFMT, wide=True))
    legs = {"wide": _captured(made[0], True) if KVFMT is not None else dec, "COGV_DECODE_WIDE=0": _captured(made[1], False),
            "8 rows": _captured(made[2], True)}
    if WFMT is not None:
        legs[f"{WFMT} wide"] = _captured(made[3], True)
    del made
    with torch.no_grad():
        ms, last = _time_legs(legs)
    cache = f"{KVFMT or '16-bit'} cache"
    w, n, e = (min(ms[k]) for k in ("wide", "COGV_DECODE_WIDE=0", "8 rows"))
    print(f"captured graph, {B} rows, {cache}: wide step {w:.2f} ms ({'gemm_rows' if wide_on else 'NOT taken: the step of the other leg'}); "
          f"COGV_DECODE_WIDE=0 step {n:.2f} ms ({n / w:.2f}x); 8-row step {e:.2f} ms; per row {w / B:.3f} / {n / B:.3f} / {e / 8:.3f} ms "
          f"(runs {['%.2f' % v for v in ms['wide']]} / {['%.2f' % v for v in ms['COGV_DECODE_WIDE=0']]} / {['%.2f' % v for v in ms['8 rows']]})", flush=True)
    a, b = last["COGV_DECODE_WIDE=0"], last["wide"]
    print(f"logits wide vs COGV_DECODE_WIDE=0 on the timed step: rel-L2 {((b - a).norm() / a.norm()).item():.3e}, "
          f"max |difference| {(b - a).abs().max().item():.3e} (max |logit| {a.abs().max().item():.3f})", flush=True)
    if WFMT is not None:
        q, dq = min(ms[f"{WFMT} wide"]), legs[f"{WFMT} wide"]
        q_bytes = sum(t.numel() * t.element_size() for t in dq.wq.tensors())
        c = last[f"{WFMT} wide"]
        print(f"captured graph, {B} rows, {cache}: {WFMT} wide step {q:.2f} ms (wide=True: gemm_rows_{'w4' if WFMT == 'mxfp4' else 'w8'}); 16-bit wide step "
              f"{w:.2f} ms ({w / q:.2f}x); COGV_DECODE_WIDE=0 step {n:.2f} ms ({n / q:.2f}x); per row {q / B:.3f} ms; {WFMT} copies {q_bytes / 1e9:.2f} GB, "
              f"{q_bytes / q / 1e9:.2f} TB/s (runs {['%.2f' % v for v in ms[f'{WFMT} wide']]})", flush=True)
        print(f"logits {WFMT} wide vs 16-bit wide on the timed step: rel-L2 {((c - b).norm() / b.norm()).item():.3e}, "
              f"max |difference| {(c - b).abs().max().item():.3e} (max |logit| {b.abs().max().item():.3f})", flush=True)
        del dq, c
        WFMT = None              # (the comparisons below build an 8-row-at-most quantized decoder)
    del legs, last
    torch.cuda.empty_cache()
if WFMT is not None:
    dec8 = GraphDecoder(model, batch=B, capacity=1152, weights=WFMT)
    with torch.no_grad():
        dec8.prefill(tokens[:, :pre], pos[:, :pre])
        dec8.capture()
        ms, last = _alternate(dec, dec8, "16-bit weights", f"{WFMT} weights")
    wq_bytes = sum(t.numel() * t.element_size() for t in dec8.wq.tensors())
    pairs = [qs for lw in dec8.wq.layers for qs in lw] + [dec8.wq.emb]
    w16_bytes = 2 * sum(q.numel() for q, _ in pairs) * (2 if WFMT == "mxfp4" else 1)       # the same matrices in 16 bits
    mq, m16 = min(ms[f"{WFMT} weights"]), min(ms["16-bit weights"])
    _report(ms, last, "16-bit weights", f"{WFMT} weights", f"{WFMT} vs 16-bit",
            f"; {WFMT} copies {wq_bytes / 2 ** 30:.2f} GiB; weight bytes per second {w16_bytes / m16 / 1e9:.2f} TB/s (16-bit, {w16_bytes / 1e9:.2f} GB) / "
            f"{wq_bytes / mq / 1e9:.2f} TB/s ({WFMT}, {wq_bytes / 1e9:.2f} GB)")
    if KVFMT is not None:
        del dec
        dec = dec8                                               # the 8-bit cache is compared on the same weights
    del dec8
if KVFMT is not None:
    wname = f"{WFMT or '16-bit'} weights"
    deck = GraphDecoder(model, batch=B, capacity=1152, weights=WFMT, kv=KVFMT)
    with torch.no_grad():
        deck.prefill(tokens[:, :pre], pos[:, :pre])
        deck.capture()
        ms, last = _alternate(dec, deck, f"{wname}, 16-bit cache", f"{wname}, {KVFMT} cache")
    b16 = sum(c.numel() * c.element_size() for c in dec.caches)
    b8 = sum(t.numel() * t.element_size() for t in deck.kv8.tensors())
    _report(ms, last, f"{wname}, 16-bit cache", f"{wname}, {KVFMT} cache", f"{KVFMT} cache vs 16-bit cache",
            f"; cache bytes per step {b16 / 1e9:.3f} GB -> {b8 / 1e9:.3f} GB")
    del deck
del model, dec
torch.cuda.empty_cache()
if os.environ.get("MB_DECODE_GRAPH_ONLY") == "1":
    sys.exit(0)
for kv in (True, False):
    model = FP16_Module(GPT2Model(L, V, h, heads, 0.1, 0.1, 0.1, 1089, 1089, False, kv_cache=kv).cuda(), dtype=torch.bfloat16,
                        keep_half_outputs=True).eval()
    with torch.no_grad():
        torch.cuda.synchronize(); t0 = time.time()
        logits, *mems = model(tokens[:, :pre], pos[:, :pre], 0, None, None, 0)
        torch.cuda.synchronize(); t_pre = time.time() - t0
        for t in range(pre, pre + 4):                       # warm-up steps
            logits, *mems = model(tokens[:, t:t + 1], pos[:, t:t + 1], 0, None, None, 0, *mems)
        torch.cuda.synchronize(); t0 = time.time()
        for t in range(pre + 4, pre + steps):
            logits, *mems = model(tokens[:, t:t + 1], pos[:, t:t + 1], 0, None, None, 0, *mems)
        torch.cuda.synchronize(); dt = (time.time() - t0) / (steps - 4)
    print(f"kv_cache={kv}: prefix of {pre} tokens {t_pre*1e3:.1f} ms; decode {dt*1e3:.2f} ms/token at memory length ~{pre}", flush=True)
    del model, mems, logits
    torch.cuda.empty_cache()
