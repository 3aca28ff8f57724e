"""Single-token decode latency of the 4B model with a 1024-position memory: the captured HIP-graph decode step
(generation.GraphDecoder), eager K/V-cache memories (kv_cache=True) and the reference-style layer-input memories (every
step re-projects K and V of the whole memory).  `--weights e4m3`: in the same run, the captured step on the 8-bit copies of the
weights (GraphDecoder(weights="e4m3")) next to the 16-bit one -- ms per token of each, and the relative L2 / largest difference
of their logits on the step that was timed."""
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
tokens, pos = tokens.expand(B, -1).contiguous(), pos.expand(B, -1).contiguous()
dec = GraphDecoder(model, batch=B, capacity=1152)
with torch.no_grad():
    dec.prefill(tokens[:, :pre], pos[:, :pre])
    for mode in ("eager fixed-capacity step", "captured graph"):
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
if "--weights" in sys.argv:
    fmt = sys.argv[sys.argv.index("--weights") + 1]
    dec8 = GraphDecoder(model, batch=B, capacity=1152, weights=fmt)
    with torch.no_grad():
        dec8.prefill(tokens[:, :pre], pos[:, :pre])
        dec8.capture()
        while dec8.length < dec.length:                          # the same history (and memory length) as the 16-bit decoder
            dec8.step(tokens[:, pre:pre + 1], pos[:, pre:pre + 1])
        ms, last = {}, {}
        for rep in range(2):                                     # 16-bit, 8-bit, and once more each: the order must not matter
            for name, d in (("16-bit", dec), (fmt, dec8)):
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
        lg16, lg8 = last["16-bit"], last[fmt]
    w8_bytes = sum(t.numel() * t.element_size() for t in dec8.w8.tensors())
    print(f"captured graph, 16-bit weights: {min(ms['16-bit']):.2f} ms/token; {fmt} weights: {min(ms[fmt]):.2f} ms/token "
          f"({min(ms['16-bit']) / min(ms[fmt]):.2f}x; runs {['%.2f' % v for v in ms['16-bit']]} / {['%.2f' % v for v in ms[fmt]]})"
          + (f" (batch {B})" if B > 1 else "") + f"; 8-bit copies {w8_bytes / 2 ** 30:.2f} GiB", flush=True)
    print(f"logits {fmt} vs 16-bit on the timed step: rel-L2 {((lg8 - lg16).norm() / lg16.norm()).item():.3e}, "
          f"max |difference| {(lg8 - lg16).abs().max().item():.3e} (max |logit| {lg16.abs().max().item():.3f})", flush=True)
    del dec8
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
