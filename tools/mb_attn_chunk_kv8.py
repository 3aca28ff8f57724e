"""Device time of the chunk attention on the 8-bit cache (cogv_attention_decode_chunk_kv8) against what it replaces, by HIP
events: H = 40 heads, capacity 1408, m = 8 tokens per cache row, B = 1 and B = 3 cache rows, bf16, *pos = 1000.  Arms, each the
key-split launch with its combine launch:
    chunk_kv8   one ops.attention_decode_chunk_kv8 call                      (8-bit cache, B * 8 rows)
    8 x kv8     eight ops.attention_decode_kv8 calls at pos ... pos + 7      (8-bit cache, B rows each)
    chunk_16    one ops.attention_decode_chunk call                          (16-bit cache, B * 8 rows)
Every arm is captured as a HIP graph of REPS repetitions (the host's launch cost stays out of the reading) and the graphs are
replayed in turn, ROUNDS times, inside one process; per arm the median over the rounds and the spread (min ... max) of the time
of ONE repetition are printed.  Run the process three times for the run-to-run spread."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cogview_amd import ops

H, CAP, M, POS, REPS, ROUNDS = 40, 1408, 8, 1000, 20, 15
dt = torch.bfloat16
hp = H * 64


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); g.replay(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


for B in (1, 3):
    gen = torch.Generator().manual_seed(B)
    qkv = torch.randn((B, M, 3 * hp), generator=gen).to(dt).cuda()
    rows = [qkv[:, j:j + 1].contiguous() for j in range(M)]
    cache16 = torch.randn((B, CAP, 2 * hp), generator=gen).to(dt).cuda()
    q8 = torch.zeros((B, 2, H, CAP, 64), dtype=torch.uint8, device="cuda")
    s8 = torch.ones((B, 2, H, CAP), dtype=torch.float32, device="cuda")
    ops.kv_quantize_e4m3(cache16, q8, s8, 0)
    pos = [torch.tensor([POS + j], dtype=torch.int64, device="cuda") for j in range(M)]

    def chunk_kv8():
        ops.attention_decode_chunk_kv8(qkv, (q8, s8), pos[0], H)

    def eight_kv8():
        for j in range(M):
            ops.attention_decode_kv8(rows[j], (q8, s8), pos[j], H)

    def chunk_16():
        ops.attention_decode_chunk(qkv, cache16, pos[0], H)

    arms = {"chunk_kv8": graph_of(chunk_kv8), "8 x kv8": graph_of(eight_kv8), "chunk_16": graph_of(chunk_16)}
    for g in arms.values():
        replay_us(g)
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, g in arms.items():
            times[k].append(replay_us(g))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f"B={B} H={H} capacity={CAP} m={M} pos={POS} bf16, us per call (median of {ROUNDS} rounds of {REPS}; min ... max): "
          + "; ".join(f"{k} {med[k]:.1f} ({min(v):.1f} ... {max(v):.1f})" for k, v in times.items())
          + f"; chunk_kv8 = {med['chunk_kv8'] / med['8 x kv8']:.3f} of 8 x kv8, {med['chunk_kv8'] / med['chunk_16']:.3f} of chunk_16", flush=True)
