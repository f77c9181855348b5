"""The stream contract, made observable: "every call is asynchronous on the given hipStream_t" (INTEGRATION.md), with
torch's current stream as that stream for every wrapper of aggforce_amd/_kernels.py.

On torch's default stream a launch that drops its stream argument, a memset on another stream, a side stream that does
not wait for the caller's, or a hidden host synchronisation all give the right answer.  Here a call is made on a
non-default stream `s` BEHIND A GATE: a bounded busy kernel (torch.cuda._sleep, calibrated with events; a chain of
matmuls if _sleep does not scale) that holds `s` for at least ten times what the call takes.  The call's floating-point
inputs hold POISON (another valid data set of the same shape, dtype and scale) and receive their true values by a
`copy_` that is queued on `s` behind the gate.  So

* work that is ordered on `s` runs after the copy and gives the reference result bit for bit;
* work that escaped to another stream runs at once, on poison, and its result differs;
* a call that waits for the stream returns only when the gate has run out: its end event has then fired.

Index operands (group tables, pair lists, trees, frame indices, pins) are built before the gate and never poisoned: a
misrouted kernel reads wrong values, never outside an allocation.  Nothing here can fault; the only race is the
canary's, which reads valid memory that another stream writes later.

Every case of a group shares one gate; before it the group runs once ungated on `s` with all outputs alive, so that the
gated pass allocates nothing for the first time, and then once on the poison, so that cached workspaces and recycled
blocks hold nothing a misrouted second-stage kernel could get the right answer from.  `t_warm` (wall time of call +
synchronise on `s`, all one-time costs paid by a first untimed call) is measured before the gate is sized and never
taken from the gated run."""
import json
import os
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report_path():
    """stream_contract.json beside dispatch_coverage.json: in the scratch directory that
    tests/test_gpu_zz_coverage.py names (None if that test no longer names one: then no report is written)."""
    import re

    try:
        with open(os.path.join(ROOT, "tests", "test_gpu_zz_coverage.py")) as fh:
            found = re.search(r'out_dir = os\.path\.join\(ROOT, "([^"]+)"\)', fh.read())
    except OSError:
        found = None
    return os.path.join(ROOT, found.group(1), "stream_contract.json") if found else None


GATE_FACTOR = 10.0     # gate >= GATE_FACTOR x t_warm: a misrouted kernel finishes inside the gate on a busy machine
GATE_MAX_S = 0.5       # no gate is longer; a group that needs more must shrink its shapes
GATE_MIN_S = 0.02      # floor: host jitter between two Python statements stays far below it
HEADROOM = 1.25        # requested / required gate length (calibration error)

_state = {"calibration": None, "stream": None, "other": None, "cases": {}, "canary": {}}


def bits(t):
    """The bytes of a tensor (NaN == NaN), as tests/test_gpu_layouts.py compares them."""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).clone()
    if t.dtype == torch.float64:
        return t.view(torch.int64).clone()
    return t.clone()


def flat(out):
    """The tensors of a call's result (a tensor, None, or nested tuples / lists of them), in order."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flat(o)]
    raise TypeError(f"a case returned {type(out)}: return tensors (host values: wrap them in torch.as_tensor)")


def same_bits(a, b):
    """Equal byte for byte; either side may already be the `bits` of its tensors."""
    a, b = [bits(t) for t in flat(a)], [bits(t) for t in flat(b)]
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def default_poison(x):
    """Another data set of x's shape, dtype and scale: a convex mix of x with itself shifted by one element (positive
    data stays positive, finite data finite)."""
    f = x.reshape(-1)
    if f.numel() < 2:
        return (x * 1.5 + 0.25).clone()
    return (0.25 * f + 0.75 * f.roll(1)).reshape(x.shape).clone()


# ------------------------------------------------------------------ streams and the gate
def stream():
    """The non-default stream the contract is tested on (one per session)."""
    if _state["stream"] is None:
        _state["stream"] = torch.cuda.Stream()
        _state["other"] = torch.cuda.Stream()
    return _state["stream"]


def other_stream():
    stream()
    return _state["other"]


def _matmul_chain(n):
    a = _state.setdefault("mm", torch.full((1024, 1024), 1.0 / 1024, device="cuda"))
    b = a
    for _ in range(int(n)):
        b = a @ b


def _time_gate(fn, units, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        fn(units)
        e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def calibrate():
    """{kind, seconds per unit, intercept}: the gate kernel timed with events at two lengths on an idle stream; no
    clock rate is assumed.  torch.cuda._sleep if its length follows its argument, else a chain of matmuls."""
    if _state["calibration"] is not None:
        return _state["calibration"]
    st = stream()
    torch.cuda.synchronize()
    tried = []
    for kind, fn, lo, hi in (("sleep", lambda c: torch.cuda._sleep(int(c)), 2_000_000, 8_000_000),
                             ("matmul", _matmul_chain, 50, 200)):
        try:
            _time_gate(fn, lo, st)  # code loading
            t_lo = min(_time_gate(fn, lo, st) for _ in range(2))
            t_hi = min(_time_gate(fn, hi, st) for _ in range(2))
        except Exception as exc:  # _sleep missing in this build
            tried.append({"kind": kind, "error": repr(exc)})
            continue
        slope = (t_hi - t_lo) / (hi - lo)
        tried.append({"kind": kind, "units": [lo, hi], "seconds": [t_lo, t_hi]})
        if slope > 0 and t_hi > 2.0 * t_lo - 1e-4 and t_hi > 1e-4:
            # check the extrapolation once at a gate-sized length
            cal = {"kind": kind, "s_per_unit": slope, "intercept_s": max(0.0, t_lo - slope * lo), "tried": tried}
            want = 0.05
            got = _time_gate(fn, (want - cal["intercept_s"]) / slope, st)
            cal["check"] = {"requested_s": want, "measured_s": got}
            if 0.5 * want < got < 2.0 * want:
                cal["s_per_unit"] *= got / want if got < want else 1.0  # never undershoot
                cal["fn"] = fn
                _state["calibration"] = cal
                return cal
    raise AssertionError(f"no gate kernel whose length follows its argument: {tried}")


def gate(seconds, st):
    """Queue a busy kernel of about `seconds` on `st`; returns the pair of events around it."""
    cal = calibrate()
    assert seconds <= GATE_MAX_S * 1.0001, f"a gate of {seconds:.3f} s: shrink the case (cap {GATE_MAX_S} s)"
    units = max(1.0, (seconds - cal["intercept_s"]) / cal["s_per_unit"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    cal["fn"](units)
    e1.record(st)
    return e0, e1


def gate_length(t_warm):
    """(required, requested) seconds for work whose warm call takes t_warm."""
    need = max(GATE_FACTOR * t_warm, GATE_MIN_S)
    return need, min(need * HEADROOM, GATE_MAX_S) if need <= GATE_MAX_S else need * HEADROOM


# ------------------------------------------------------------------ coverage bookkeeping
_dump_bytes = [1 << 16]


def _totals():
    """{mangled name: (demangled name, launches since the library was loaded)}: _lib.coverage(names=True, total=True)
    in ONE pass of aggf_coverage_dump (a buffer kept large enough).  The dump demangles every kernel the process has
    ever launched -- milliseconds late in a long session, so its cost is measured and added to the gate."""
    import ctypes

    from aggforce_amd import _lib

    lib = _lib.load()
    while True:
        buf = ctypes.create_string_buffer(_dump_bytes[0])
        need = lib.aggf_coverage_dump(buf, _dump_bytes[0])
        if need < _dump_bytes[0]:
            break
        _dump_bytes[0] = 2 * need + 4096
    out = {}
    for line in buf.value.decode().splitlines():
        mangled, pretty, _cnt, tot = line.split("\t")
        out[mangled] = (pretty, int(tot))
    return out


def family_of(pretty):
    """Demangled kernel name without template arguments, return type and parameter list."""
    name = pretty.replace("void ", "").split("(")[0]
    return name.split("<")[0].strip()


def _launched_between(before, after):
    """Kernels launched between two readings of the counters: demangled, without return type and parameter list."""
    return sorted({p.replace("void ", "").split("(")[0] for k, (p, n) in after.items() if n > before.get(k, ("", 0))[1]})


# ------------------------------------------------------------------ the method
def run_behind_gate(cases, monkeypatch=None):
    """`cases`: one case or a list that shares one gate.  A case is an object with
      name         its id in the report
      build()      -> (floats, call): `floats` the list of floating-point input tensors holding the TRUE data (or pairs
                   (true, poison) where the default poison would not be a valid input); call(*floats) makes the call
                   under test on the current stream and returns its output tensors
      families     substrings of the (demangled) names of kernels the gated call must launch
      synchronises None, or the reason the wrapper waits for the stream by contract (then it is the last of its group
                   and the two `query()` assertions are skipped)
      env          {name: value} set through monkeypatch around all runs of the case
      cleanup      optional: called once after the gated run has been synchronised
    Returns {name: kernels launched in the gated run}."""
    if not isinstance(cases, (list, tuple)):
        cases = [cases]
    s = stream()
    calibrate()
    for c in cases[:-1]:
        assert not c.synchronises, f"{c.name}: a case that waits for the stream must be the last of its group"
    prepared = []
    for c in cases:
        with _env(c, monkeypatch):
            floats, call = c.build()
            true = [f[0] if isinstance(f, tuple) else f for f in floats]
            poison = [f[1] if isinstance(f, tuple) else default_poison(f) for f in floats]
            for t, p in zip(true, poison):
                assert p.shape == t.shape and p.dtype == t.dtype and bool(torch.isfinite(p).all()), c.name
            # 1. reference on the default stream; the poison gives another result
            ref = [bits(t) for t in flat(call(*[t.clone() for t in true]))]
            torch.cuda.synchronize()
            bad = [bits(t) for t in flat(call(*[p.clone() for p in poison]))]
            torch.cuda.synchronize()
            assert true, f"{c.name}: no floating-point input to poison"
            assert not same_bits(ref, bad), f"{c.name}: the poison gives the reference result: the case can see nothing"
            # 2. warm-up on s: one-time costs, then the timed call
            with torch.cuda.stream(s):
                bufs = [t.clone() for t in true]
                s.synchronize()
                for timed in (False, True):
                    t0 = time.perf_counter()
                    out = call(*bufs)
                    s.synchronize()
                    t_warm = time.perf_counter() - t0
                    assert same_bits(out, ref), f"{c.name}: on a non-default stream (no gate) the result differs"
                del out
            prepared.append((c, true, poison, call, ref, t_warm))
    torch.cuda.synchronize()

    # 3. the gated run
    t_sum = sum(p[5] for p in prepared)
    need, want = gate_length(t_sum)
    # the host reads the launch counters once per case while the gate runs: that time (not the library's) is added whole,
    # with a margin of two, to what the contract requires
    _totals()
    t0 = time.perf_counter()
    _totals()
    t_book = time.perf_counter() - t0
    want += 2.0 * len(cases) * t_book
    assert want <= GATE_MAX_S * 1.0001, (f"{[c.name for c in cases]}: t_warm {t_sum * 1e3:.1f} ms needs a gate of "
                                         f"{want:.2f} s (cap {GATE_MAX_S} s): shrink the shapes or split the group")
    buffers = [[p.clone() for p in poison] for _, _, poison, _, _, _ in prepared]
    torch.cuda.synchronize()
    # Rehearsal, still without a gate: the whole group once on s with every output kept alive, as the gated pass keeps
    # them.  The caching allocator's pool of s then holds a block for every allocation the gated pass makes, in the same
    # order; a first-time device allocation in the middle of the gated pass may wait for the device, which is the
    # allocator's business and not the call's.
    with torch.cuda.stream(s):
        held = []
        for (c, true, _, call, ref, _), bufs in zip(prepared, buffers):
            with _env(c, monkeypatch):
                for b, t in zip(bufs, true):
                    b.copy_(t)
                held.append(call(*bufs))
        s.synchronize()
        for (c, _, _, _, ref, _), out in zip(prepared, held):
            assert same_bits(out, ref), f"{c.name}: in the rehearsal of its group the result differs"
        del held, out
        # The LAST pass on s before the gate runs on the poison, results dropped: the workspaces cached for s and the
        # blocks its allocator hands out again then hold intermediates of the poison, not of the true data -- a second
        # stage (a slab sum, a finishing kernel) that escaped from s would otherwise read stale but CORRECT partials.
        for (_, _, poison, _, _, _), bufs in zip(prepared, buffers):
            for b, p in zip(bufs, poison):
                b.copy_(p)
        held = []
        for (c, _, _, call, _, _), bufs in zip(prepared, buffers):
            with _env(c, monkeypatch):
                held.append(call(*bufs))
        s.synchronize()
        del held
    outs, launched, waited, host_s = [], {}, [], {}
    before = _totals()
    with torch.cuda.stream(s):
        e0, e1 = gate(want, s)
        for (c, true, _, call, _, _), bufs in zip(prepared, buffers):
            with _env(c, monkeypatch):
                for b, t in zip(bufs, true):
                    b.copy_(t, non_blocking=True)
                t0 = time.perf_counter()
                out = call(*bufs)
                # directly after the call returns the gate must still be running and hold the stream
                done = s.query() or e1.query()
                t1 = time.perf_counter()
                now = _totals()
                host_s[c.name] = (t1 - t0, time.perf_counter() - t1)
                launched[c.name], before = _launched_between(before, now), now
            outs.append(out)
            if not c.synchronises and done:
                waited.append(c.name)
        quiet = not any(c.synchronises for c in cases)
        if quiet and not waited:
            time.sleep(max(t_sum, 1e-3))  # a misrouted kernel has now certainly run, on poison
            still = not s.query()
        else:
            still = True
        s.synchronize()
    gate_s = e0.elapsed_time(e1) * 1e-3
    for (c, _, _, _, _, t_warm) in prepared:
        _state["cases"][c.name] = {"t_warm_s": t_warm, "group_t_warm_s": t_sum, "gate_requested_s": want,
                                   "gate_measured_s": gate_s, "gate_over_t_warm": gate_s / t_sum,
                                   "counter_read_s": t_book, "gated_call_host_s": host_s[c.name][0],
                                   "gated_counter_read_host_s": host_s[c.name][1],
                                   "families": sorted({family_of(k) for k in launched[c.name]}),
                                   "kernels": launched[c.name], "synchronises": c.synchronises}
    write_report()
    for c in cases:  # (pooled flags and the like go back now that the stream is idle)
        if getattr(c, "cleanup", None):
            c.cleanup()
    assert gate_s >= need, f"the gate lasted {gate_s:.3f} s, {need:.3f} s were required: calibration {calibrate()}"
    assert not waited, (f"{waited}: the gate had run out when the call returned -- the call waited for the stream "
                        f"(gate {gate_s * 1e3:.0f} ms, t_warm {t_sum * 1e3:.2f} ms)")
    assert still, (f"{[c.name for c in cases]}: the stream ran dry within t_warm of the last call: a call waited for the "
                   "stream, or the gate did not hold")
    wrong = [c.name for (c, _, _, _, ref, _), out in zip(prepared, outs) if not same_bits(out, ref)]
    assert not wrong, f"{wrong}: behind the gate the result differs from the default-stream result (work off the stream)"
    for c in cases:
        for fam in c.families:
            assert any(fam in n for n in launched[c.name]), (c.name, fam, launched[c.name])
    return launched


class _env:
    def __init__(self, case, monkeypatch):
        self.env, self.mp = getattr(case, "env", None) or {}, monkeypatch

    def __enter__(self):
        if self.env:
            assert self.mp is not None, "a case with an environment hook needs the monkeypatch fixture"
            self.ctx = self.mp.context()
            m = self.ctx.__enter__()
            for k, v in self.env.items():
                m.setenv(k, v)

    def __exit__(self, *exc):
        if self.env:
            self.ctx.__exit__(*exc)


def write_report():
    cal = {k: v for k, v in (_state["calibration"] or {}).items() if k != "fn"}
    path = report_path()
    if path is None:
        return
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"calibration": cal, "gate_factor": GATE_FACTOR, "gate_max_s": GATE_MAX_S, "canary": _state["canary"],
                       "cases": _state["cases"]}, fh, indent=1)
    except OSError:
        pass


def gated_families():
    """Kernel families launched behind a gate so far in this session."""
    return sorted({f for c in _state["cases"].values() for f in c["families"]})
