"""CPU: what the four device entry points (generate_on_device, generate_batch_on_device, DeviceGenerator, DeviceFiller) ask of
their SamplingDecoder -- constructor keywords, sampler arguments, start / capture / generate, in order -- on a recording fake
installed as decoder.SamplingDecoder, and the refusal of every unsupported combination before the first tensor allocation.
The expected traces are written out by hand; the refusal table states, per call site, what each violated condition raises."""
import types

import pytest
import torch

from cogview_amd.generation import (DeviceFiller, DeviceGenerator, GraphDecoder, SamplingDecoder, decoder, generate_batch_on_device,
                                    generate_on_device, inverse_prompt_score_on_device, plan_device_fill)
from tests.generation_cases import ToyIds

IDS = ToyIds(32, 16)
BOI1 = IDS["[BOI1]"]
MODEL = types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8, dtype=torch.float16)))


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


@pytest.fixture
def log(monkeypatch):
    """Installs the fake; yields the list its instances record into (the instances themselves are log.decoders)."""
    class Log(list):
        pass

    log = Log()
    log.decoders = []

    class Fake:
        def __init__(self, model, **kw):
            assert model is MODEL
            log.append(("ctor", kw))
            log.decoders.append(self)
            self.batch, self.cap = kw["batch"], kw["capacity"]
            self.tok = torch.zeros((self.batch, 1), dtype=torch.long)
            self.graph = self.given = self.offset = self.scores = self.out_tokens = None

        def enable_sampling(self, temperature=1.0, top_k=0, top_p=0.0, allow=None, seed=0, out_tokens=None, out_base=0, given=None):
            log.append(("enable_sampling", float(temperature), int(top_k), float(top_p), tuple(allow), int(seed), tuple(out_tokens.shape),
                        int(out_base), given is not None))
            self.offset = torch.zeros(1, dtype=torch.int64)
            self.scores = torch.zeros(self.batch, dtype=torch.float32)
            self.out_tokens, self.given = out_tokens, given

        def start(self, tokens, position_ids, attention_mask=0):
            assert not torch.is_grad_enabled()
            log.append(("start", tuple(tokens.shape), position_ids.tolist(), tuple(attention_mask.shape),
                        None if self.given is None else self.given.tolist()))
            self.out_tokens.fill_(7)
            self.scores.fill_(-1.5)

        def start_ragged(self, tokens, position_ids, pads):
            assert not torch.is_grad_enabled()
            log.append(("start_ragged", tuple(tokens.shape), position_ids.tolist(), list(pads)))
            self.out_tokens.fill_(7)
            self.scores.fill_(-1.5)

        def capture(self):
            log.append(("capture", self.graph))
            self.graph = object()

        def generate(self, n):
            assert not torch.is_grad_enabled()
            log.append(("generate", n))

    monkeypatch.setattr(decoder, "SamplingDecoder", Fake)
    return log


# ---------------------------------------------------------------------------------------------------------- generate_on_device
T2I = [40, BOI1, -3, -3, -3]
T2I_HEAD = [("ctor", dict(batch=3, capacity=64, weights=None)),
            ("enable_sampling", 1.0, 1, 0.0, (0, 32), 5, (3, 3), 2, False),
            ("start", (1, 2), [[0, 1]], (1, 1, 2, 2), None)]


def test_generate_on_device_trace(log):
    tokens, scores = generate_on_device(MODEL, torch.tensor(T2I), _args(), tokenizer=IDS, seed=5)
    assert log == T2I_HEAD + [("capture", None), ("generate", 2)]
    assert tokens.tolist() == [[40, BOI1, 7, 7, 7]] * 3 and scores.tolist() == [-1.5] * 3
    assert scores is not log.decoders[0].scores


def test_generate_on_device_without_capture(log):
    generate_on_device(MODEL, torch.tensor(T2I), _args(), tokenizer=IDS, seed=5, capture=False)
    assert log == T2I_HEAD + [("generate", 2)]


def test_generate_on_device_run_of_one_mark(log):
    tokens, _ = generate_on_device(MODEL, torch.tensor([40, BOI1, -3]), _args(), tokenizer=IDS, seed=5)
    assert log == [("ctor", dict(batch=3, capacity=64, weights=None)),
                   ("enable_sampling", 1.0, 1, 0.0, (0, 32), 5, (3, 1), 2, False),
                   ("start", (1, 2), [[0, 1]], (1, 1, 2, 2), None)]                    # no capture, no generate
    assert tokens.tolist() == [[40, BOI1, 7]] * 3


def test_generate_on_device_formats(log):
    generate_on_device(MODEL, torch.tensor(T2I), _args(), tokenizer=IDS, weights="e4m3", kv="e4m3")
    assert log[0] == ("ctor", dict(batch=3, capacity=64, weights="e4m3", kv="e4m3"))


# ---------------------------------------------------------------------------------------------------- generate_batch_on_device
def _prompts():
    return [torch.tensor([40, BOI1, -2, -2]), torch.tensor([40, 41, BOI1, -2, -2])]


def test_generate_batch_on_device_trace(log):
    tokens, scores = generate_batch_on_device(MODEL, _prompts(), _args(temperature=0.5, top_k=3, top_p=0.25), tokenizer=IDS, seed=2)
    assert log == [("ctor", dict(batch=4, capacity=64, weights=None, ragged=True)),
                   ("enable_sampling", 0.5, 3, 0.25, (0, 32), 2, (4, 2), 3, False),
                   ("start_ragged", (2, 3), [[0, 0, 1], [0, 1, 2]], [1, 0]),
                   ("capture", None), ("generate", 1)]
    assert [t.tolist() for t in tokens] == [[[40, BOI1, 7, 7]] * 2, [[40, 41, BOI1, 7, 7]] * 2]
    assert scores.tolist() == [[-1.5, -1.5]] * 2


def test_generate_batch_on_device_formats_and_no_capture(log):
    generate_batch_on_device(MODEL, _prompts(), _args(), tokenizer=IDS, capture=False, weights="e4m3", kv="e4m3")
    assert log[0] == ("ctor", dict(batch=4, capacity=64, weights="e4m3", kv="e4m3", ragged=True))
    assert [e[0] for e in log] == ["ctor", "enable_sampling", "start_ragged", "generate"]


def test_one_prompt_is_generate_on_device(log):
    tokens, scores = generate_batch_on_device(MODEL, [torch.tensor(T2I)], _args(), tokenizer=IDS, seed=5)
    assert log == T2I_HEAD + [("capture", None), ("generate", 2)]                     # the plain decoder: no ragged keyword
    assert [t.tolist() for t in tokens] == [[[40, BOI1, 7, 7, 7]] * 3] and scores.tolist() == [[-1.5] * 3]


# -------------------------------------------------------------------------------------------------------------- DeviceGenerator
def _rearm(log, call, first_start):
    """The shared second-call and re-arm cases of the two reusable forms; `call(args)` runs one more call."""
    call(_args())
    assert [e[0] for e in log] == ["ctor", "enable_sampling", first_start, "capture", "generate", first_start, "generate"]
    dec, graph = log.decoders[0], log.decoders[0].graph
    dec.offset.fill_(7)                                                    # the draws made so far
    call(_args(temperature=0.75))
    assert len(log.decoders) == 1
    assert [e[0] for e in log[7:]] == ["enable_sampling", first_start, "capture", "generate"]
    assert log[7][1:5] == (0.75, 1, 0.0, (0, 32))
    assert dec.offset.tolist() == [7]                                      # the generator keeps counting across the re-arm
    assert log[9] == ("capture", None) and dec.graph is not graph         # the old graph was dropped before the new capture
    return dec


def test_device_generator_trace(log):
    gen = DeviceGenerator(MODEL, _args(), rows=4, capacity=64, seed=3)
    assert log == [] and gen.dec is None
    tokens, scores = gen(_prompts(), tokenizer=IDS)
    assert log == [("ctor", dict(batch=4, capacity=64, weights=None, ragged=True)),
                   ("enable_sampling", 1.0, 1, 0.0, (0, 32), 3, (4, 64), 0, False),
                   ("start_ragged", (2, 3), [[0, 0, 1], [0, 1, 2]], [1, 0]),
                   ("capture", None), ("generate", 1)]
    assert [t.tolist() for t in tokens] == [[[40, BOI1, 7, 7]] * 2, [[40, 41, BOI1, 7, 7]] * 2]
    assert scores.tolist() == [[-1.5, -1.5]] * 2
    dec = _rearm(log, lambda args: gen(_prompts(), args=args, tokenizer=IDS), "start_ragged")
    assert gen.dec is dec and gen.out is dec.out_tokens and tuple(gen.out.shape) == (4, 64)


def test_device_generator_formats_and_no_capture(log):
    gen = DeviceGenerator(MODEL, _args(), rows=4, capacity=64, capture=False, weights="e4m3", kv="e4m3")
    gen(_prompts(), tokenizer=IDS)
    assert log[0] == ("ctor", dict(batch=4, capacity=64, weights="e4m3", kv="e4m3", ragged=True))
    assert [e[0] for e in log] == ["ctor", "enable_sampling", "start_ragged", "generate"]


# ----------------------------------------------------------------------------------------------------------------- DeviceFiller
FILL = [40, BOI1, -1, 3, -1, 5]


def test_device_filler_trace(log):
    filler = DeviceFiller(MODEL, _args(), seed=4, capacity=64)
    assert log == [] and filler.dec is None
    row = filler(MODEL, torch.tensor(FILL), _args(), tokenizer=IDS)
    table = plan_device_fill(FILL, IDS, 56)["given"]
    assert table == [-1, -1, -1, 3, -1, -1]
    assert log == [("ctor", dict(batch=1, capacity=64, weights=None)),
                   ("enable_sampling", 1.0, 1, 0.0, (0, 32), 4, (1, 64), 0, True),
                   ("start", (1, 2), [[0, 1]], (1, 1, 2, 2), table + [-1] * 58),
                   ("capture", None), ("generate", 2)]
    assert row.tolist() == [[40, BOI1, 7, 7, 7, 5]]                           # the trailing given id comes from seq
    assert filler.scores.tolist() == [-1.5] and filler.scores is not filler.dec.scores
    dec = _rearm(log, lambda args: filler(MODEL, torch.tensor(FILL), args, tokenizer=IDS), "start")
    assert filler.dec is dec and filler.given is dec.given and tuple(filler.given.shape) == (64,)


def test_device_filler_formats_and_no_capture(log):
    filler = DeviceFiller(MODEL, _args(), capacity=64, capture=False, weights="e4m3", kv="e4m3")
    filler(MODEL, torch.tensor(FILL), _args(), tokenizer=IDS)
    assert log[0] == ("ctor", dict(batch=1, capacity=64, weights="e4m3", kv="e4m3"))
    assert [e[0] for e in log] == ["ctor", "enable_sampling", "start", "generate"]


# --------------------------------------------------------------------------------------------------------------- refusal matrix
def _no_alloc(monkeypatch):
    """any tensor factory the decoders use fails the test: a refusal comes before the first allocation"""
    def boom(*a, **k):
        raise AssertionError("a tensor was allocated before the refusal")
    for name in ("zeros", "ones", "empty", "arange", "full"):
        monkeypatch.setattr(torch, name, boom)


def _gpt(dtype):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(1, 64, 512, 8, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


NIE = NotImplementedError
SEQ = torch.tensor([40, BOI1, -1, -1])
SEQS = [torch.tensor([40, BOI1, -1, -1]), torch.tensor([40, 41, BOI1, -1, -1])]
ROWS = torch.tensor([[40] * 1030])
FEATURES = {"none": {}, "weights": dict(weights="e4m3"), "kv": dict(kv="e4m3"), "weights+kv": dict(weights="e4m3", kv="e4m3")}



def _table():
    """(id, site, call(model, args) -> None, model, args keywords, mp size, exception, match), one per call site x feature set x
    violated condition.  A float32 model without kv= / several prompts is not refused by the callers (weights= on a float32 model is
    the decoder constructor's to refuse, where the transformer is at hand), so those cells have no row."""
    rows = []

    def add(site, feat, cond, call, exc, pat, model=None, akw=None, mp=1):
        rows.append(pytest.param(call, model, akw or {}, mp, exc, pat, id=f"{site}-{feat}-{cond}"))

    # the decoder constructors: no args, so no sparse conditions; a decoder without a feature refuses nothing
    for cls in (GraphDecoder, SamplingDecoder):
        feats = {**{k: v for k, v in FEATURES.items() if k != "none"}, "ragged": dict(ragged=True)}
        for feat, kw in feats.items():
            def call(model, args, cls=cls, kw=kw):
                cls(model, batch=2, **kw)
            add(cls.__name__, feat, "mp=2", call, NIE, "model parallelism", model="m16", mp=2)
            add(cls.__name__, feat, "float32", call, NIE, "float32", model="m32")
            for name in kw:
                if name != "ragged":
                    def bad(model, args, cls=cls, kw=kw, name=name):
                        cls(model, batch=2, **{**kw, name: "int8"})
                    add(cls.__name__, feat, f"bad {name}", bad, ValueError, f"{name}=", model="m16")
    # the four entry points; the two batch forms are the `ragged` feature set, alone and with the formats
    sites = {"generate_on_device": (False, lambda model, args, **kw: generate_on_device(model, SEQ, args, tokenizer=IDS, **kw)),
             "DeviceFiller": (False, lambda model, args, **kw: DeviceFiller(model, args, **kw)),
             "generate_batch_on_device": (True, lambda model, args, **kw: generate_batch_on_device(model, SEQS, args, tokenizer=IDS, **kw)),
             "DeviceGenerator": (True, lambda model, args, **kw: DeviceGenerator(model, args, rows=2, **kw))}
    for site, (ragged, entry) in sites.items():
        for feat, kw in FEATURES.items():
            feat = {"none": "ragged"}.get(feat, "ragged+" + feat) if ragged else feat

            def call(model, args, entry=entry, kw=kw):
                entry(model, args, **kw)
            add(site, feat, "is_sparse=2", call, NIE, "sparse generation.*filling_sequence", akw=dict(is_sparse=2))
            add(site, feat, "is_sparse=1", call, ValueError, "is_sparse==2", akw=dict(is_sparse=1))
            add(site, feat, "mp=2", call, NIE, "model parallelism > 1.*filling_sequence", mp=2)
            if "kv" in kw:
                add(site, feat, "float32", call, NIE, "float32.*filling_sequence", model="m32")
            elif ragged:
                add(site, feat, "float32", call, NIE, "float32", model="m32")
            for name in kw:
                def bad(model, args, entry=entry, kw=kw, name=name):
                    entry(model, args, **{**kw, name: "fp4"})
                add(site, feat, f"bad {name}", bad, ValueError, f"{name}=")
    # a call of the reusable forms with other args, and the scorer
    calls = {"DeviceGenerator.__call__": ("gen", "filling_sequence", lambda gen, args: gen(SEQS, args=args, tokenizer=IDS)),
             "DeviceFiller.__call__": ("filler", "filling_sequence", lambda filler, args: filler(filler.model, SEQ, args, tokenizer=IDS)),
             "inverse_prompt_score_on_device": (None, "inverse_prompt_score",
                                                lambda model, args: inverse_prompt_score_on_device(model, ROWS, args, tokenizer=IDS))}
    for site, (obj, use, call) in calls.items():
        add(site, "none", "is_sparse=2", call, NIE, f"sparse generation.*{use}", model=obj, akw=dict(is_sparse=2))
        add(site, "none", "is_sparse=1", call, ValueError, "is_sparse==2", model=obj, akw=dict(is_sparse=1))
        add(site, "none", "mp=2", call, NIE, f"model parallelism > 1.*{use}", model=obj, mp=2)
    return rows


@pytest.fixture(scope="module")
def things():
    m16 = _gpt(torch.float16)
    return {None: None, "m16": m16, "m32": _gpt(torch.float32), "gen": DeviceGenerator(m16, _args(), rows=2, capacity=64),
            "filler": DeviceFiller(m16, _args(), capacity=64)}


@pytest.mark.parametrize("call, model, akw, mp, exc, pat", _table())
def test_refusal_matrix(monkeypatch, things, call, model, akw, mp, exc, pat):
    from cogview_amd.mpu import initialize
    args = _args(**akw)
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: mp)
    _no_alloc(monkeypatch)
    with pytest.raises(exc, match=pat):
        call(things[model], args)
