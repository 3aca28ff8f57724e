"""Bits of every device generation entry point, for comparing two trees of this package (a refactor of the host side must not move
one): generate_on_device (nb 1 and 4), generate_batch_on_device (3 x 1 and 2 x 4), DeviceGenerator and DeviceFiller (two calls and
a re-armed third) on the 2-layer h = 1024 model of tests/test_batch_generation_gpu.py, formats {16-bit, kv8, w8, kv8+w8}, captured
and eager, fixed seeds.
    python tools/generation_bits.py dump TREE OUT.pt     tokens and the bit patterns of the scores of the package under TREE
    python tools/generation_bits.py compare A.pt B.pt    one line per result; exit status 1 if any differs"""
import os, sys, types
import torch

if sys.argv[1] == "compare":
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    assert list(a) == list(b)
    bad = 0
    for k in a:
        (ta, sa), (tb, sb) = a[k], b[k]
        tok = len(ta) == len(tb) and all(torch.equal(x, y) for x, y in zip(ta, tb))
        sc = torch.equal(sa, sb)
        bad += not (tok and sc)
        n = sum(x.numel() for x in ta)
        print(f"   {k}: {n} tokens {'equal' if tok else 'DIFFER'}, {sa.numel()} score bit patterns {'equal' if sc else 'DIFFER'} (first {sa.view(-1)[0].item() & 0xffffffff:08x})")
    print(f"RESULT: {len(a)} results, {bad} differ" + ("" if bad else ": tokens and score bits identical"))
    sys.exit(1 if bad else 0)

assert sys.argv[1] == "dump"
ROOT = os.path.abspath(sys.argv[2])
sys.path.insert(0, ROOT)
import cogview_amd
assert os.path.abspath(cogview_amd.__file__).startswith(ROOT + os.sep), cogview_amd.__file__
from cogview_amd.generation import DeviceFiller, DeviceGenerator, generate_batch_on_device, generate_on_device
from tests.test_batch_generation_gpu import _h1024, _h1024_seqs

model, ids, ctxs, n_img = _h1024()
args = lambda: types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)
greedy = lambda: types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)
res = {}


def put(key, tokens, scores):
    tokens = tokens if isinstance(tokens, (list, tuple)) else [tokens]
    res[key] = ([t.cpu().clone() for t in tokens], scores.detach().cpu().contiguous().view(torch.int32).clone())


def window(ctx, pattern):
    return torch.tensor(ctx + pattern, dtype=torch.long, device="cuda")


W1 = [-1, -1, 5, -1, 7, 9, -1, -1, -1, 11, -1, -1, 3, -1, -1, -1, 2, 4]
W2 = [-1, 6, -1, -1, -1, 8, -1, 1, -1, -1]
FORMATS = {"16-bit": {}, "kv8": dict(kv="e4m3"), "w8": dict(weights="e4m3"), "kv8+w8": dict(kv="e4m3", weights="e4m3")}
for fname, fmt in FORMATS.items():
    for cap in (True, False):
        tag = f"{fname} {'captured' if cap else 'eager'}"
        for nb in (1, 4):
            seq = _h1024_seqs(ctxs, (0,), nb)[0]
            put(f"{tag} | generate_on_device nb {nb}", *generate_on_device(model, seq.clone(), args(), tokenizer=ids, seed=1234, capture=cap, **fmt))
        for which, nb in (((0, 1, 2), 1), ((1, 2), 4)):
            seqs = _h1024_seqs(ctxs, which, nb)
            put(f"{tag} | generate_batch_on_device {len(which)} x {nb}",
                *generate_batch_on_device(model, [s.clone() for s in seqs], args(), tokenizer=ids, seed=1234, capture=cap, **fmt))
        gen = DeviceGenerator(model, args(), rows=2, capacity=64, seed=77, capture=cap, **fmt)
        put(f"{tag} | DeviceGenerator call 1", *gen([s.clone() for s in _h1024_seqs(ctxs, (2, 0), 1)], tokenizer=ids))
        put(f"{tag} | DeviceGenerator call 2", *gen([s.clone() for s in _h1024_seqs(ctxs, (1, 2), 1, run=9)], tokenizer=ids))
        put(f"{tag} | DeviceGenerator call 3 (re-armed, greedy)", *gen([s.clone() for s in _h1024_seqs(ctxs, (0, 1), 1)], args=greedy(), tokenizer=ids))
        fill = DeviceFiller(model, args(), seed=55, capacity=64, capture=cap, **fmt)
        for i, (c, w) in enumerate(((2, W1), (1, W2))):
            out = fill(model, window(ctxs[c], w), args(), tokenizer=ids)
            put(f"{tag} | DeviceFiller window {i + 1}", out, fill.scores)
        out = fill(model, window(ctxs[0], W1), greedy(), tokenizer=ids)
        put(f"{tag} | DeviceFiller window 3 (re-armed, greedy)", out, fill.scores)
torch.cuda.synchronize()
torch.save(res, sys.argv[3])
print(f"{ROOT}: {len(res)} results saved to {sys.argv[3]}")
