"""Run a case off the default stream and compare it, bit for bit, with its run on the default stream.
A helper of tests/test_gpu_streams.py and tests/test_streams_cpu.py, not a test.

aerognn/core.py promises that every launch goes to the caller's current HIP stream. Everything the
library computes is deterministic, so a call under `with torch.cuda.stream(s)` must give the bits of the
same call on the default stream. A launch (or an async copy or memset inside an entry point) that drops
its stream argument lands on the null stream, torch's default stream, and is invisible there.

A case is a callable that builds (fn, inputs): `inputs` is a dict of the device tensors fn reads,
parameters included; fn() returns a dict of output tensors (a training case: outputs and leaf
gradients). fn may be called any number of times and must give the same bits every time; it may add
tensors to `inputs` during its first call (the output gradients of a training step, whose shapes the
first call finds). check() runs

  first call     fn() on the default stream, not measured: it pays what is paid once
  reference      fn() on the default stream; outputs kept on the host, with the core.PROF trace and the
                 wall time t_host of the call
  warm-up        fn() on a side stream s (one that runs next to the default stream, concurrent_stream)
                 with nothing else going on: allocator blocks and library
                 workspaces settle; compared already
  late inputs    every input is poisoned (floats NaN, integers 0: never an out-of-range index), then on
                 s a spin of max(50 ms, 3 t_host), the copies that restore the inputs, and fn(). When fn
                 returns on the host, s must still be busy (else the run proves nothing and fails as
                 inconclusive): every launch was then issued while the inputs still held poison, and one
                 that does not wait for the work queued before it on s reads poison, or runs before what
                 it depends on
  busy default   a spin of max(50 ms, 3 x the warm-up's wall time) on the default stream, then fn() and
                 the copies of its outputs to the host on s. The default stream must still be busy
                 after them: a launch that went to it delivers after the outputs were read. The only
                 variant for a case that blocks the host (syncs=True)

Before each variant fn() runs twice on s with the inputs poisoned: its outputs must differ from the
reference (a case that cannot tell poison from truth shows nothing), and the allocator blocks that the
variant's intermediates and outputs will take then hold those wrong bits and not the right ones of an
earlier run, which a launch that ran too early, or whose result came too late, would otherwise show.

Bits are compared through integer views of the same width, so NaN payloads and the sign of zero count.
The core.PROF traces ([tag, cost] per launch) of all runs must be equal: the same kernels ran.
While a case runs every entry point of include/aerognn.h that takes a stream is wrapped on the L.lib()
object and the ones called are recorded in OBSERVED[case name].

Library state that fn reads besides tensors (the device fault word) is poisoned and restored through the
optional attributes fn.poison_state() / fn.restore_state(); fn.after() runs after each run has been
waited for. Such a case is syncs=True: the host calls cannot be ordered on a stream.
"""
import contextlib
import os
import re
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aerognn.h")
MIN_DELAY_MS = 50.0
MAX_DELAY_MS = 2000.0   # a case that needs a longer spin is split
OBSERVED = {}           # case name -> the stream-taking entry points its runs called
TIMES = {}              # case name -> {"t_host_ms", "late_delay_ms", "busy_delay_ms"}

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def stream_entries(header=HEADER):
    """Every function of include/aerognn.h whose last parameter is `void* stream`, in header order."""
    from aerognn import _header
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return [m[2] for m in _header._PROTO.finditer(text) if re.search(r"\bvoid\s*\*\s*stream\s*$", m[3])]


# ------------------------------------------------------------------------------- poison
def poisonable(t):
    return t.is_floating_point() or t.dtype in (torch.int32, torch.int64)


def poison_(t):
    """t filled in place with the safe poison: NaN for a floating tensor, 0 for an int32 / int64 one
    (edge ids, row pointers, permutations, batch vectors of zeros stay in range). Shape, dtype and
    strides are t's own; elements of the storage outside a strided t are left alone."""
    if not poisonable(t):
        raise TypeError(f"no safe poison for a {t.dtype} tensor (bytes may hold anything: keep them out of `inputs`)")
    with torch.no_grad():
        t.fill_(float("nan") if t.is_floating_point() else 0)
    return t


def reachable_tensors(root, prefix=""):
    """{path: tensor} of the poisonable device tensors a closure reads: through function closures, modules
    (parameters and buffers), dicts, lists, tuples and the plain index holders of aerognn.graph (Level,
    Pooling) and types.SimpleNamespace. Byte buffers (packed weights, descriptor tables) are left out."""
    import types
    found, seen = {}, set()

    def walk(o, path, depth):
        if id(o) in seen or depth > 6:
            return
        seen.add(id(o))
        if torch.is_tensor(o):
            if o.is_cuda and poisonable(o) and o.numel():
                found[path] = o
        elif isinstance(o, torch.nn.Module):
            for n, p in list(o.named_parameters()) + list(o.named_buffers()):
                walk(p, f"{path}.{n}", depth + 1)
        elif isinstance(o, dict):
            for k, v in o.items():
                walk(v, f"{path}[{k}]", depth + 1)
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                walk(v, f"{path}[{i}]", depth + 1)
        elif isinstance(o, types.FunctionType):
            for name, cell in zip(o.__code__.co_freevars, o.__closure__ or ()):
                try:
                    walk(cell.cell_contents, f"{path}{name}", depth + 1)
                except ValueError:  # an empty cell
                    pass
        elif isinstance(o, types.SimpleNamespace) or type(o).__module__ == "aerognn.graph":
            for k, v in vars(o).items():
                walk(v, f"{path}.{k}", depth + 1)

    walk(root, prefix, 0)
    return found


# ------------------------------------------------------------------------------- bits
def bits(t):
    """A host copy of t as integers of its element width."""
    t = t.detach().cpu().contiguous()
    if t.is_floating_point() or t.dtype == torch.bool:
        t = t.view(_INT_VIEW[t.element_size()])
    return t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def differing(got, ref):
    """Names whose bits differ between two {name: bits} dicts (a missing or extra name counts)."""
    return sorted(k for k in set(got) | set(ref) if k not in got or k not in ref or not same_bits(got[k], ref[k]))


# ------------------------------------------------------------------------------- recording
@contextlib.contextmanager
def recording(name):
    """Counting wrappers over every stream-taking entry point, as instance attributes of the L.lib()
    object (they shadow _Lib.__getattr__ and the timed launchers); restored afterwards."""
    from aerognn import _lib as L
    lib = L.lib()
    seen = OBSERVED.setdefault(name, set())
    saved = {}
    for entry in stream_entries():
        had = entry in vars(lib)
        inner = getattr(lib, entry)
        saved[entry] = (had, inner)

        def counted(*args, _inner=inner, _entry=entry):
            seen.add(_entry)
            return _inner(*args)
        setattr(lib, entry, counted)
    try:
        yield seen
    finally:
        for entry, (had, inner) in saved.items():
            if had:
                setattr(lib, entry, inner)
            else:
                delattr(lib, entry)


# ------------------------------------------------------------------------------- sleep
def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, from one timed spin (HIP events)."""
    torch.cuda.synchronize()
    torch.cuda._sleep(1_000_000)  # (the first call also reads the clock rate)
    n = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(n)
    b.record()
    b.synchronize()
    return n / a.elapsed_time(b)


def concurrent_stream(rate, tries=8):
    """A side stream that the device runs next to the default stream. The runtime maps streams to a few
    hardware queues, and a stream that shares the default stream's queue runs in submission order with
    it: a launch that lost its stream would then be ordered by accident and nothing would show. Each
    candidate is tried once: with the default stream spinning, a small fill on it must complete."""
    for _ in range(tries):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        torch.cuda._sleep(int(20 * rate))  # on the default stream
        with torch.cuda.stream(s):
            torch.zeros(8, device="cuda")
        s.synchronize()
        beside = torch.cuda.default_stream().query() is False
        torch.cuda.synchronize()
        if beside:
            return s
    raise AssertionError(f"none of {tries} side streams ran next to the default stream")


def _delay_cycles(ms, rate, what):
    assert ms <= MAX_DELAY_MS, f"{what}: needs a spin of {ms:.0f} ms (> {MAX_DELAY_MS:.0f} ms): split the case"
    return int(ms * rate)


# ------------------------------------------------------------------------------- the check
class _Runner:
    def __init__(self, fn, inputs):
        from aerognn import core
        self.core, self.fn, self.inputs = core, fn, inputs
        self.saved = None

    def call(self):
        """(outputs, trace, host seconds) of one fn() on the current stream, not waited for."""
        core = self.core
        core._fault.update(event=None, n=0, dirty=False, word=0)  # no poll copy in one run and not in another
        core.PROF = []
        try:
            t0 = time.perf_counter()
            out = self.fn()
            dt = time.perf_counter() - t0
            trace = [[tag, None if cost is None else list(cost)] for tag, cost, *_ in core.PROF]
        finally:
            core.PROF = None
        assert out and all(torch.is_tensor(v) for v in out.values())
        return out, trace, dt

    def after(self):
        f = getattr(self.fn, "after", None)
        if f is not None:
            f()

    def save(self):
        self.saved = {k: t.detach().clone() for k, t in self.inputs.items()}

    def poison(self):
        for t in self.inputs.values():
            poison_(t)
        f = getattr(self.fn, "poison_state", None)
        if f is not None:
            f()
        torch.cuda.synchronize()

    def restore(self, state=True):
        """The copies that put the true inputs back, on the current stream."""
        with torch.no_grad():
            for k, t in self.inputs.items():
                t.copy_(self.saved[k])
        f = getattr(self.fn, "restore_state", None)
        if f is not None and state:
            f()

    def scribble(self, s, ref, what):
        """fn() on s over poisoned inputs, twice: each must differ from the reference. Leaves the inputs
        poisoned. Twice, because the blocks a run gets depend on what the run before still holds (its
        outputs, until they are dropped): after two runs both sets of blocks hold poisoned results, and
        none the right bits of an earlier run, whichever set the variant's run then takes."""
        self.poison()
        for _ in range(2):
            with torch.cuda.stream(s):
                out, _, _ = self.call()
            s.synchronize()
            got = {k: bits(v) for k, v in out.items()}
            del out
            self.after()
            assert differing(got, ref), f"{what}: poisoned inputs give the reference's bits: the case shows nothing"


def check(name, build, rate, s, monkeypatch, syncs=False):
    """Run the case `build` as the module docstring says; returns the reference's {name: bits}. rate:
    cycles_per_ms(); s: concurrent_stream(rate). monkeypatch switches core.CHECK_FAULTS off for the duration (agn_fault_status is a
    device synchronisation after every hand-off launch) and keeps the fault poll's exit hooks from
    being registered by this process."""
    from aerognn import _lib as L
    from aerognn import core
    monkeypatch.setattr(core, "CHECK_FAULTS", False)
    for k, v in list(core._fault.items()):
        monkeypatch.setitem(core._fault, k, v)
    monkeypatch.setitem(core._fault, "hooked", True)
    fn, inputs = build()
    r = _Runner(fn, inputs)
    stateful = hasattr(fn, "poison_state")
    assert syncs or not stateful, f"{name}: library state cannot be restored in stream order"
    torch.cuda.synchronize()
    assert L.fault_status(reset=True) == 0
    if stateful:
        fn.restore_state()
    with recording(name):
        # the first call pays what is paid once (code objects, operator registration, packed tables and
        # their blocking uploads) and draws a training case's output gradients: kept out of t_host
        out = r.call()
        del out
        torch.cuda.synchronize()
        r.after()
        # reference
        out, trace, t_host = r.call()
        torch.cuda.synchronize()
        ref = {k: bits(v) for k, v in out.items()}
        del out
        r.after()
        assert inputs, f"{name}: no inputs"
        r.save()
        # warm-up on s
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            out, tr, _ = r.call()
        s.synchronize()
        t_warm = time.perf_counter() - t0
        bad = differing({k: bits(v) for k, v in out.items()}, ref)
        del out  # (a run's outputs are dropped before the next run allocates)
        r.after()
        assert not bad, f"{name} warm-up on a side stream: {bad} differ from the default stream's bits"
        assert tr == trace, f"{name} warm-up: another launch sequence than on the default stream"
        late_ms = max(MIN_DELAY_MS, 3e3 * t_host)
        busy_ms = max(MIN_DELAY_MS, 3e3 * t_warm)
        TIMES[name] = dict(t_host_ms=1e3 * t_host, t_warm_ms=1e3 * t_warm, late_delay_ms=None if syncs else late_ms,
                           busy_delay_ms=busy_ms)
        print(f"[streams] {name}: t_host {1e3 * t_host:.2f} ms, warm-up {1e3 * t_warm:.2f} ms, delays: late inputs "
              f"{'-' if syncs else f'{late_ms:.0f} ms'}, busy default stream {busy_ms:.0f} ms")

        if not syncs:
            cyc = _delay_cycles(late_ms, rate, f"{name} late inputs")
            r.scribble(s, ref, name)  # (leaves the inputs poisoned, device idle)
            with torch.cuda.stream(s):
                torch.cuda._sleep(cyc)
                r.restore()
                out, tr, _ = r.call()
                done = s.query()
            s.synchronize()
            got = {k: bits(v) for k, v in out.items()}
            del out
            r.after()
            assert done is False, (f"{name} late inputs: inconclusive, the stream was idle when the call returned "
                                   f"(spin {late_ms:.0f} ms)")
            bad = differing(got, ref)
            assert not bad, f"{name} late inputs: {bad} differ: a launch did not wait for the work queued before it"
            assert tr == trace, f"{name} late inputs: another launch sequence"

        cyc = _delay_cycles(busy_ms, rate, f"{name} busy default stream")
        r.scribble(s, ref, name)
        r.restore()
        torch.cuda.synchronize()
        torch.cuda._sleep(cyc)  # on the default stream
        with torch.cuda.stream(s):
            out, tr, _ = r.call()
            got = {k: bits(v) for k, v in out.items()}  # .cpu() inside the block waits for s alone
            del out
        done = torch.cuda.default_stream().query()
        torch.cuda.synchronize()
        r.after()
        assert done is False, (f"{name} busy default stream: inconclusive, the default stream was idle when the "
                               f"outputs had been read (spin {busy_ms:.0f} ms)")
        bad = differing(got, ref)
        assert not bad, f"{name} busy default stream: {bad} differ: a launch went to the default stream"
        assert tr == trace, f"{name} busy default stream: another launch sequence"
    if stateful:
        fn.poison_state()
    assert L.fault_status(reset=True) == 0
    return ref


# ------------------------------------------------------------------------------- launch_cases
def launch_case(name, setenv):
    """A case of launch_cases.CASES as a builder of (fn, inputs): fn is launch_cases.step without its
    waits. The output gradients of a training step are drawn at the first call (on the default stream,
    before the reference run; its outputs give the shapes) and join `inputs`; later calls draw nothing
    and block nowhere."""
    import launch_cases as LC

    def build():
        builder, kw, env = LC.CASES[name]
        for k, v in env.items():
            setenv(k, v)
        fwd, leaves = builder(**kw)
        train = kw.get("train", True)
        inputs = reachable_tensors(fwd)
        for k, t in leaves.items():
            if not any(t is u for u in inputs.values()):
                inputs["leaf " + k] = t
        gs = {}

        def fn():
            if not train:
                with torch.no_grad():
                    return {k: v.detach() for k, v in fwd().items()}
            for t in leaves.values():
                t.grad = None
            outs = fwd()
            if not gs:
                for i, (k, o) in enumerate(outs.items()):
                    gs[k] = torch.randn(o.shape, generator=LC._gen(7 + i)).to(o.dtype).to(LC.DEV)
                    inputs["g " + k] = gs[k]
            torch.autograd.backward(list(outs.values()), [gs[k] for k in outs])
            res = {k: v.detach() for k, v in outs.items()}
            for k, t in leaves.items():
                assert t.grad is not None, k
                res["d " + k] = t.grad
            return res
        return fn, inputs
    return build
