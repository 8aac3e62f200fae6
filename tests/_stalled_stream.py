"""A stalled stream, and the scenario the tests/test_gpu_stalled_stream_*.py files run behind it.

``Stall(S, ms)`` puts device work of about ``ms`` milliseconds at the front of the non-blocking side stream ``S`` and records an event
directly behind it; ``still_stalled()`` is ``not event.query()``.  The stall is ``torch.cuda._sleep`` (a kernel that ends by itself
after a number of clock ticks), calibrated once per process with two timing events; were it not to stall on a runtime, a fixed-length
chain of matmuls takes its place.  Nothing here waits for the host: a stalled stream always drains on its own, after 500 ms at the most.

``run_scenario`` is the one scenario (reference on the default stream, poison, P then Q on the stalled stream, Q from a second stream
meanwhile, bit-equality); a test describes its entry point as two ``Call``s that share one handle."""
import time

import numpy as np
import torch

FLOOR_MS, CAP_MS, FACTOR = 20.0, 500.0, 10.0
_PROBE_CYCLES = 20_000_000
_unit = None  # ("sleep", cycles per ms) | ("matmul", matmuls per ms, the operand)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate():
    global _unit
    if _unit is None:
        torch.cuda._sleep(1000)  # (the first call loads the kernel)
        ms = _timed(lambda: torch.cuda._sleep(_PROBE_CYCLES))
        if ms >= 1.0:
            _unit = ("sleep", _PROBE_CYCLES / ms)
        else:  # _sleep does not stall here: a chain of matmuls of fixed length does
            m = torch.ones((2048, 2048), dtype=torch.float32, device="cuda")
            torch.mm(m, m)
            chain = 50
            ms = _timed(lambda: [torch.mm(m, m) for _ in range(chain)])
            _unit = ("matmul", chain / ms, m)
        print(f"stall calibration: {_unit[0]}, {_unit[1]:.4g} units per ms")
    return _unit


def stall_ms_for(enqueue_ms):
    """The stall of a case whose warm-up enqueue sequence took ``enqueue_ms`` of host time: 10 times that, within [20, 500] ms."""
    return float(min(CAP_MS, max(FLOOR_MS, FACTOR * enqueue_ms)))


class Stall:
    def __init__(self, stream, ms):
        assert 0.0 < ms <= CAP_MS
        unit = _calibrate()
        self.stream, self.ms = stream, ms
        with torch.cuda.stream(stream):
            if unit[0] == "sleep":
                torch.cuda._sleep(int(ms * unit[1]))
            else:
                for _ in range(max(1, int(ms * unit[1]))):
                    torch.mm(unit[2], unit[2])
            self.end = torch.cuda.Event()
            self.end.record(stream)

    def still_stalled(self):
        return not self.end.query()


_pair = None


def side_streams():
    """Two non-blocking side streams, the same two for the whole process, that are seen to run independently of each other.

    The runtime maps its streams onto a few hardware queues (4 by default), and two streams that share a queue run one behind the other:
    a call on the second stream would then wait for the first one's stall although no event and no host wait ties them.  So the pair is
    probed once: a short stall on S, one tiny kernel on U, and U must drain while S is still stalled.  torch hands out streams from a
    pool, so another candidate for U costs no new stream; if none of 8 is independent of S the caller fails (it does not skip)."""
    global _pair
    if _pair is None:
        S = torch.cuda.Stream()
        for _ in range(8):
            U = torch.cuda.Stream()
            torch.cuda.synchronize()
            stall = Stall(S, FLOOR_MS)
            with torch.cuda.stream(U):
                torch.zeros(1, device="cuda")
            U.synchronize()
            independent = stall.still_stalled()
            S.synchronize()
            if independent:
                _pair = (S, U)
                break
        assert _pair is not None, "no second stream runs while the first one is stalled: every candidate shares its hardware queue"
    return _pair


class Call:
    """One call of an entry point on buffers of the scenario's choosing.

    host:    name -> pinned host tensor with the real contents of a device INPUT buffer (an arena that is also written: its whole image)
    outputs: name -> (shape, dtype, poison) of a device buffer the call only writes; poison is a float (NaN) or, for 2-byte types, an
             int16 bit pattern the result cannot contain
    run:     (buffers: name -> device tensor) -> list of device tensors, the result; enqueues on torch's CURRENT stream
    check:   (list of host tensors, the result) -> None; holds it to the kind's float64 reference and bars"""

    def __init__(self, host, outputs, run, check):
        self.host = {k: (v if v.is_pinned() else v.pin_memory()) for k, v in host.items()}
        self.outputs, self.run, self.check = outputs, run, check

    def poisoned(self):
        bufs = {}
        for k, v in self.host.items():
            if v.dtype.is_floating_point or v.dtype.is_complex:
                bufs[k] = torch.full(v.shape, float("nan"), dtype=v.dtype, device="cuda")
            else:  # bytes (a feature arena): 0xFF, a NaN in float32 and binary16; PCM: the most negative value, which no test signal holds
                bufs[k] = torch.full(v.shape, 0xFF if v.dtype == torch.uint8 else torch.iinfo(v.dtype).min, dtype=v.dtype, device="cuda")
        for k, (shape, dtype, poison) in self.outputs.items():
            if isinstance(poison, int):
                bufs[k] = torch.full(shape, poison, dtype=torch.int16, device="cuda").view(dtype)
            else:
                bufs[k] = torch.full(shape, poison, dtype=dtype, device="cuda")
        return bufs

    def upload(self, bufs):  # on the current stream, from pinned memory: the host does not wait
        for k, v in self.host.items():
            bufs[k].copy_(v, non_blocking=True)


def host_bits(tensors):
    """Device tensors -> their bytes on the host (the caller has synchronised, or the copy does)."""
    real = [torch.view_as_real(t.detach()) if t.is_complex() else t.detach() for t in tensors]
    return [t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8) for t in real]


def host_values(tensors):
    return [t.detach().cpu() for t in tensors]


def same(what, got, want):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))


def run_scenario(name, P, Q, warm_rounds):
    """The scenario of DESIGN §4.12.1 for two calls P and Q that share one handle (closed over by their ``run``).

    warm_rounds: rounds of (P, Q) on the default stream until every slot of the handle's ring has made its first allocation: 8 for a
    ticketed handle (16 calls), 2 for a plan's or a resampler's ring (4 calls).  Steps 4 and 5 hold the results to the bits of step 1:
    every kind that goes through here claims that a run repeats bit for bit."""
    S, U = side_streams()
    # 1. reference: default stream, fully synchronised; the last round's host enqueue time sizes the stall
    for _ in range(warm_rounds):
        bp, bq = P.poisoned(), Q.poisoned()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.upload(bp), Q.upload(bq)
        rp, rq = P.run(bp), Q.run(bq)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    want_p, want_q = host_bits(rp), host_bits(rq)
    P.check(host_values(rp)), Q.check(host_values(rq))
    for stream in (S, U):  # the allocator's first blocks (small and large pool) of each side stream: a wrapper's torch.empty there finds them
        with torch.cuda.stream(stream):
            first_blocks = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (512, 4 << 20)]
        del first_blocks
    # 2. poison
    bp, bq, bu = P.poisoned(), Q.poisoned(), Q.poisoned()
    Q.upload(bu)
    torch.cuda.synchronize()
    # 3. on S, behind the stall
    ms = stall_ms_for(enqueue_ms)
    print(f"{name}: warm-up enqueue {enqueue_ms:.3f} ms, stall {ms:.0f} ms")
    stall = Stall(S, ms)
    with torch.cuda.stream(S):
        P.upload(bp), Q.upload(bq)
        rp = P.run(bp)
        rq = Q.run(bq)
    assert stall.still_stalled(), f"{name}: the host did not finish enqueuing P and Q while the stream was stalled ({ms:.0f} ms)"
    # 4. the same handle from a free-running stream meanwhile
    with torch.cuda.stream(U):
        ru = Q.run(bu)
    U.synchronize()
    assert stall.still_stalled(), f"{name}: the call on the second stream waited for the stalled one ({ms:.0f} ms)"
    with torch.cuda.stream(U):  # (the download must not order itself behind S either)
        got_u = host_bits(ru)
    same(f"{name}: Q on the second stream", got_u, want_q)
    # 5.
    S.synchronize()
    assert not stall.still_stalled()
    same(f"{name}: P behind the stall", host_bits(rp), want_p)
    same(f"{name}: Q behind the stall", host_bits(rq), want_q)
