"""include/smt.h, Conventions: "`stream` is a hipStream_t ... Calls are asynchronous on that stream unless documented as
synchronising."  The rest of the suite issues its work on torch's default stream, with inputs that are complete before the
first launch and results read after everything has drained; here every device entry point runs on a side stream that is
BUSY, with inputs that exist only behind the work in front of it.

Part one, the table (tests/bounds_cases.py through tests/stream_order_cases.py, one seed, unwritten float outputs NaN):

    A.build(deferred=True)            # the arena holds DECOYS of the inputs (tests/arena.py), fully synchronised
    with torch.cuda.stream(side):
        torch.cuda._sleep(DELAY)      # side is busy
        A.arrive()                    # the inputs -- and the prefill of the outputs -- exist only behind the sleep
        rc = call()                   # the table's closure, unchanged; its stream is torch's current one: side
        snap = A.buf.clone()          # a consumer on the same stream, no host synchronisation
    side.synchronize(); check and verify on snap

A launch, memset or copy that is not ordered behind the caller's stream -- on stream 0, on an internal stream that was
forked without waiting for the caller's -- reads decoys or has its output overwritten by arrive(); a join that is missing
at the end of a call shows in snap for the closures that do not synchronise themselves.  Either way the case fails against
the oracle.  AD-Census batches run under SMT_OVERLAP 0 / 1 / 2, pipeline batches under SMT_PIPE_SCHEDULE 0 / 1 / 2 with one
five-pair case for schedule 2.

The library as the closure sees it is a thin proxy that, for the ONE entry under test, records at the moment the entry
returns whether the SLEEP was still running (an event recorded right behind it) and the host time since the sleep was
enqueued (closures also create, read status, copy back and destroy, which may wait: the probe sits on the entry).
Entries decided ASYNC in stream_order_cases.SYNCHRONISING must have returned while the sleep ran, entries decided SYNC
after it.  "The stream is still busy" would not do: an entry that waits first and enqueues afterwards leaves a busy
stream behind.  A call in front of the entry can wait as well -- hipFree waits for every stream of the device (the
placement search of smt_adcensus_create inside smt_pipeline_create_on), and the synchronous hipMemset / hipMemcpy of a
create wait for the sleep where the null stream shares the hardware queue of the side stream (every fourth stream with
HIP's default of four queues, GPU_MAX_HW_QUEUES: on the MI355X about one case in 25) -- so when the sleep has ended, or
a quarter of it has passed, by the time the entry is reached, the proxy puts the decoys back, sleeps and lets the inputs
arrive again: the entry itself always meets a busy stream and late inputs.

That the harness rejects a mis-streamed launch is shown on the device without touching a kernel: two stand-in entries
written in torch (out = in + 1 on the arena's tensors), one on side, which passes, one on a second torch stream, which
must be rejected.  The second stream is one that was observed to run beside a busy side (streams that share a hardware
queue are ordered by the queue; with HIP's default of four queues, GPU_MAX_HW_QUEUES, that is one pair in four).  The
same holds for the library's internal streams: an ordering defect is visible where the stream concerned has a hardware
queue of its own.

Part two, reused handles: for pipeline groups 4 .. 7 of tests/fuzz_flow_cases.py (schedules unset / 0 / 1 / 2) and the first
two groups of cblsm, crossagg, sad, ncc and asw, one handle, one warm batch on the default stream, then on a fresh side
stream behind one sleep the batches 0, 1, 2, 0 back to back -- each batch's images copied on the stream into tensors that
held reversed decoys until then, run / run_post / run_v4 through stereo_match_traditional_amd.api, every returned map
cloned on the stream -- with no host synchronisation in between: the sleep must still be running after the last enqueue.
Then every clone against FC.oracle_batch by the rules of tests/test_fuzz_flows_gpu.py, and the repeated batch 0 against
its first run byte for byte.

The delay.  torch.cuda._sleep(400_000_000) lasts 166.65 ms on the MI355X (events; 2.4e9 cycles per second); the longest
host time the probe saw between enqueuing a sleep and the return of an asynchronous entry was 7.8 ms (3.2 ms inside the
whole suite).  The sleep has to be at least ten times that long and not shorter than 50 ms: DELAY = 400_000_000 keeps a
factor of 21 and stays.  A sleep that is too short fails the assertions, it cannot pass silently.

Not held here: NULL-stream semantics, two host threads on one handle, a handle moved between streams without a
synchronisation in between, several devices, smt_adcensus_host_run (synchronising; tests/test_adcensus_host_cpu.py holds
its schedule)."""
import copy
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402
import exact_matchers as XM  # noqa: E402
import fuzz_flow_cases as FC  # noqa: E402
import stream_order_cases as SC  # noqa: E402
from prefill import flows  # noqa: E402,F401  (the fixture: the api's output tensors come prefilled)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DELAY = SC.DELAY
ENV = ("SMT_OVERLAP", "SMT_PIPE_SCHEDULE")


@pytest.fixture(scope="module")
def X(smt, O):
    return BC.Ctx(O, "cuda:0")


# ================================================================================================ part one: the table
class Probe:
    """the library as the closure of one case sees it: every function is the library's own; the entry under test is
    wrapped"""

    def __init__(self, lib, entry, standins=None):
        self._lib, self._entry, self._standins = lib, entry, standins or {}
        self.returns = []               # (the sleep still running, ms since it was enqueued) at every return of the entry
        self.rearmed = 0

    def bind(self, A, side):
        self._A, self._side = A, side
        self._decoys = A.buf.clone()

    def arm(self):
        """on torch's current stream: the decoys (again), the sleep, and behind it the inputs"""
        self._A.buf.copy_(self._decoys, non_blocking=True)
        self._t0 = time.perf_counter()
        torch.cuda._sleep(DELAY)
        self._slept = torch.cuda.Event()
        self._slept.record()
        self._A.arrive()

    def __getattr__(self, name):
        f = self._standins[name] if name in self._standins else getattr(self._lib, name)
        if name != self._entry:
            return f

        def probed(*a):
            # A call of the closure in front of the entry has waited for the sleep (hipFree in a create waits for every
            # stream; a synchronous hipMemset / hipMemcpy of a create waits where the null stream shares the hardware
            # queue of this one), or has used up a quarter of it: the entry gets a fresh one.
            if self._slept.query() or (not self.returns and 1e3 * (time.perf_counter() - self._t0) > SC.DELAY_MS / 4):
                self.arm()
                self.rearmed += 1
            rc = f(*a)
            self.returns.append((not self._slept.query(), 1e3 * (time.perf_counter() - self._t0)))
            return rc
        return probed


def run_deferred(X, name, make, params, side=None, standins=None):
    """one case on a busy stream with late inputs, checked and verified on the snapshot -> its Probe"""
    A = arena.Arena(arena.SEEDS[1], X.device)
    probe = Probe(X.lib, name, standins)
    Xp = copy.copy(X)
    Xp.lib = probe
    call, verify = make(A, Xp, **params)
    A.build(deferred=True, keep=tuple(SC.NO_DECOY.get(name, ())), decoys=SC.own_decoys(name, A))
    assert A.decoyed(), "no input differs from its decoy: the case proves nothing"
    side = torch.cuda.Stream() if side is None else side
    probe.bind(A, side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        probe.arm()
        rc = call()
        snap = A.buf.clone()
    side.synchronize()
    torch.cuda.synchronize()
    assert rc == 0, f"{name}{params}: status {rc}"
    o = A.check(snap)
    o.update(A.extra)
    verify(o)
    return probe


_CASES = SC.cases()


@pytest.mark.parametrize("name,params,env", [c[1:] for c in _CASES], ids=[c[0] for c in _CASES])
def test_entry_on_a_busy_stream_with_late_inputs(X, monkeypatch, name, params, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    probe = run_deferred(X, name, BC.ENTRIES[name], params)
    decision = SC.SYNCHRONISING[name]
    print(f"PROBE {name} {decision!r} rearmed {probe.rearmed} returns " +
          " ".join(f"{'busy' if p else 'idle'}@{ms:.3f}ms" for p, ms in probe.returns))
    assert probe.returns, f"the closure never called {name}"
    seen = f"{[(p, round(ms, 3)) for p, ms in probe.returns]}; the sleep lasts {SC.DELAY_MS:.0f} ms"
    if decision == SC.SYNC:
        assert not any(p for p, _ in probe.returns), f"{name} is documented as synchronising but returned while the sleep ran ({seen})"
    else:
        # ASYNC_WARM: the first call on a handle may wait, and the closure makes no other (the warm calls: part two)
        held = probe.returns[1:] if decision == SC.ASYNC_WARM else probe.returns
        assert all(p for p, _ in held), f"{name} is decided {decision!r} but the sleep had ended when it returned ({seen}): it waited"


def test_every_table_case_is_decided():
    assert {c[1] for c in _CASES} == set(SC.SYNCHRONISING)


# ---- the detector detects: stand-ins written in torch ---------------------------------------------------------------
def _standin(stream):
    """out = in + 1 on the arena's tensors as an "entry": on `stream`, or on torch's current stream when it is None"""
    n = 5000
    src = BC.rf((n,), 77)

    def add_one(A):
        i, o = (A.buf[A.addr(nm) - A.base:A.addr(nm) - A.base + 4 * n].view(torch.float32) for nm in ("in", "out"))
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            o.copy_(i + 1)
        return 0

    def make(A, X):
        A.inp("in", src); A.out("out", (n,), np.float32)
        return (lambda: X.lib.standin_add_one(A)), (lambda o: BC.bits_eq(o["out"], src + 1, "out"))
    return make, {"standin_add_one": add_one}


def _beside(side):
    """a torch stream that was seen to finish work while `side` was busy; None if none of eight did"""
    for _ in range(8):
        s = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(DELAY)
        with torch.cuda.stream(s):
            torch.zeros(4, device=DEV)
        s.synchronize()
        free = not side.query()
        side.synchronize()
        if free and s != side:
            return s
    return None


def test_a_standin_on_the_callers_stream_passes(X):
    make, standins = _standin(None)
    probe = run_deferred(X, "standin_add_one", make, {}, standins=standins)
    assert [p for p, _ in probe.returns] == [True] and probe.rearmed == 0, probe.returns


def test_a_standin_on_another_stream_is_rejected(X):
    """the premise of this file: torch side streams do not order against each other, so work put on another stream runs
    before the inputs have arrived"""
    side = torch.cuda.Stream()
    other = _beside(side)
    assert other is not None, "no torch stream ran beside a busy one: the premise of this file is false on this machine"
    make, standins = _standin(other)
    with pytest.raises(AssertionError, match="out: .* bytes differ from the oracle"):
        run_deferred(X, "standin_add_one", make, {}, side=side, standins=standins)
    torch.cuda.synchronize()


# ================================================================================================ part two: reused handles
def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _rev(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1)[::-1]).reshape(np.shape(a))


def _images(family, g, k, O):
    """the stacked input arrays of batch k, in the order the family's enqueue takes them"""
    if family == "crossagg":
        pairs = FC.bgr_pairs(g, k, O)
        return [np.stack([p[i] for p in pairs]) for i in ((0, 1, 2, 3) if g["gray_given"] else (0, 1))]
    pairs = FC.gray_pairs(g, k, O)
    return [np.stack([p[i] for p in pairs]) for i in (0, 1)]


def _fail(family, g, i, k, p, name, what):
    pytest.fail(f"{family} {g['name']} chain position {i} (batch {k}, P = {g['batches'][k]['P']}) pair {p} {name}: {what}", pytrace=False)


def run_chain(family, g, O, handle, enqueue, status, warm=(SC.WARM,)):
    """warm batch(es) on the default stream; then behind one sleep on a fresh side stream the batches of SC.CHAIN back to
    back with late inputs and no host synchronisation -> [{name: numpy}] per chain position"""
    arrays = {k: _images(family, g, k, O) for k in sorted(set(SC.CHAIN) | set(warm))}
    true = {k: [T(a) for a in arrays[k]] for k in arrays}
    for k in warm:
        enqueue(handle, [t.clone() for t in true[k]])
        torch.cuda.synchronize()
    status(handle)
    slots = [[T(_rev(a)) for a in arrays[k]] for k in SC.CHAIN]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    clones = []
    slept = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(DELAY)
        slept.record()
        for slot, k in zip(slots, SC.CHAIN):
            for dst, src in zip(slot, true[k]):
                dst.copy_(src, non_blocking=True)
            clones.append({n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in enqueue(handle, slot).items()})
        pending = not slept.query() and not side.query()
    side.synchronize()
    torch.cuda.synchronize()
    assert pending, f"{family} {g['name']}: the sleep had ended after the last enqueue: a call of the chain waited"
    status(handle)
    got = [{n: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for n, t in c.items()} for c in clones]
    for name in got[0]:
        a, b = got[0][name], got[-1][name]
        if isinstance(a, np.ndarray) and a.tobytes() != b.tobytes():
            pytest.fail(f"{family} {g['name']}: batch 0 run again at the end of the chain, {name}: {FC.first_diff(b, a)}", pytrace=False)
    return got


def _compare(family, g, O, got, names):
    """bit for bit: got[name][p] against the oracle's per-pair array names[name]"""
    for i, k in enumerate(SC.CHAIN):
        outs, _ = FC.oracle_batch(family, g, k, O)
        for p, o in enumerate(outs):
            for name, key in names.items():
                a, w = got[i][name][p], np.ascontiguousarray(o[key])
                if a.shape != w.shape or a.dtype != w.dtype or a.tobytes() != w.tobytes():
                    _fail(family, g, i, k, p, name, FC.first_diff(a, w))


def _groups(family):
    return [FC.groups(family)[i] for i in SC.FLOW_GROUPS[family]]


def _gid(g):
    return g["name"]


@pytest.mark.parametrize("g", _groups("pipeline"), ids=_gid)
def test_pipeline_chain(flows, O, monkeypatch, g):
    smt = flows
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import QUIRK_FIX_RIGHT_ARM_STRIDE, SMT_ERR_REF_UB
    assert g["schedule"] == FC.PIPE_SCHEDULES[FC.groups("pipeline").index(g) % 4]
    if g["schedule"] is None:
        monkeypatch.delenv("SMT_PIPE_SCHEDULE", raising=False)
    else:
        monkeypatch.setenv("SMT_PIPE_SCHEDULE", g["schedule"])                   # read when the handle is created
    pipe = smt.Pipeline(g["H"], g["W"], g["D"], DEV, quirks=QUIRK_FIX_RIGHT_ARM_STRIDE if g["fix_stride"] else 0)

    def status(pipe):
        try:
            pipe.status()
        except SmtError as e:                                                    # the rule of tests/test_fuzz_flows_gpu.py
            if g["fix_stride"] or e.status != SMT_ERR_REF_UB:
                raise

    def enqueue(pipe, t):
        dl, dr, cls, counts = pipe.run(*t)
        pl, pr, pcls, pcounts, last = pipe.run_post(*t)
        return dict(run_dl=dl, run_dr=dr, run_cls=cls, run_counts=counts, post_dl=pl, post_dr=pr, post_cls=pcls,
                    post_counts=pcounts, post_last=last)
    try:
        got = run_chain("pipeline", g, O, pipe, enqueue, status)
    finally:
        pipe.close()
    _compare("pipeline", g, O, got, dict(run_dl="lr", run_dr="dr", run_cls="cls", run_counts="counts", post_dl="sp", post_dr="dr",
                                         post_cls="cls", post_counts="counts", post_last="med"))


@pytest.mark.parametrize("g", _groups("cblsm"), ids=_gid)
def test_cblsm_chain(flows, O, g):
    f = flows.CBLSMFlow(g["H"], g["W"], g["D"], DEV, tau=g["tau"], max_length=g["max_length"], sec_length=g["sec_length"])

    def enqueue(f, t):
        dl, dr = f.run(*t)
        pl, pr, cls, counts = f.run_post(*t)
        return dict(run_dl=dl, run_dr=dr, post_dl=pl, post_dr=pr, post_cls=cls, post_counts=counts, v4_dl=f.run_v4(*t))
    try:
        got = run_chain("cblsm", g, O, f, enqueue, lambda f: f.status())
    finally:
        f.close()
    _compare("cblsm", g, O, got, dict(run_dl="dl", run_dr="dr", post_dl="post_fin", post_dr="dr", post_cls="post_cls",
                                      post_counts="post_counts", v4_dl="v4"))


@pytest.mark.parametrize("g", _groups("crossagg"), ids=_gid)
def test_crossagg_chain(flows, O, g):
    smt = flows
    f = smt.CrossAggFlow(g["H"], g["W"], g["D"], DEV, L1=g["L1"], L2=g["L2"], t1=g["t1"], t2=g["t2"], num_iters=g["num_iters"],
                         gate=g["gate"])

    def enqueue(f, t):
        dl, dr = f.run(*t)
        ol, _ = f.run(*t, views=smt.VIEW_LEFT)
        _, orr = f.run(*t, views=smt.VIEW_RIGHT)
        ll, lr_, cls, counts = f.run(*t, lr_check=True)
        pl, pr, pcls, pcounts = f.run_post(*t)
        return dict(run_dl=dl, run_dr=dr, left_only=ol, right_only=orr, lr_dl=ll, lr_dr=lr_, lr_cls=cls, lr_counts=counts,
                    post_dl=pl, post_dr=pr, post_cls=pcls, post_counts=pcounts)
    try:
        got = run_chain("crossagg", g, O, f, enqueue, lambda f: f.status())
    finally:
        f.close()
    _compare("crossagg", g, O, got, dict(run_dl="dl", run_dr="dr", left_only="dl", right_only="dr", lr_dl="lr", lr_dr="dr",
                                         lr_cls="cls", lr_counts="counts", post_dl="post_fin", post_dr="dr", post_cls="post_cls",
                                         post_counts="post_counts"))


@pytest.mark.parametrize("g", _groups("sad"), ids=_gid)
def test_sad_chain(flows, O, g):
    f = flows.SADFlow(g["H"], g["W"], g["D"], DEV, winsize=g["winsize"])

    def enqueue(f, t):
        return dict(zip(("dl", "dr", "last", "cls"), f.run(*t)))
    try:
        got = run_chain("sad", g, O, f, enqueue, lambda f: None)
    finally:
        f.close()
    _compare("sad", g, O, got, dict(dl="dl", dr="dr", last="last", cls="cls"))


@pytest.mark.parametrize("g", _groups("ncc"), ids=_gid)
def test_ncc_chain(flows, O, g):
    """costs under the bound of the form that ran, maps by the reference's rule on the call's own costs and against O.ncc
    (tests/test_fuzz_flows_gpu.py).  The handle's tables grow to the largest batch seen and that growth may wait (smt.h):
    the largest batch is a warm batch too."""
    smt = flows
    win, D, H, W = g["winSize"], g["D"], g["H"], g["W"]
    f = smt.NCCFlow(H, W, D, DEV, winSize=win)
    largest = max(range(3), key=lambda k: g["batches"][k]["P"])

    def enqueue(f, t):
        out = {}
        for form in g["forms"]:
            f.set_form(form)
            out[f"disp{form}"], out[f"cost{form}"] = f.run(*t, want_cost=True)
            out[f"ran{form}"] = smt.ncc_last_form()                              # a host variable: no device work, no wait
        return out
    try:
        got = run_chain("ncc", g, O, f, enqueue, lambda f: None, warm=(SC.WARM, largest) if largest != SC.WARM else (SC.WARM,))
    finally:
        f.close()
    border = np.ones((H, W), bool)
    border[win:H - win, win:W - win] = False
    for i, k in enumerate(SC.CHAIN):
        outs, _ = FC.oracle_batch("ncc", g, k, O)
        for form in g["forms"]:
            disp, cost, ran = got[i][f"disp{form}"], got[i][f"cost{form}"], got[i][f"ran{form}"]
            if not border.all() and ran != (form or FC.ncc_rule(2 * win + 1, D)):
                _fail("ncc", g, i, k, "all", f"form {form}", f"ran form {ran}")
            for p, o in enumerate(outs):
                if not ((disp[p][border] == 0).all() and (cost[p][border].view(np.uint64) == 0).all()):
                    _fail("ncc", g, i, k, p, f"form {form}", "border pixels must hold map 0 and cost +0.0")
                if "exact" not in o:
                    continue
                try:
                    XM.check_ncc(cost[p], o["exact"], o["flat"], o["sentinel"], win, "loop" if ran == FC.NCC_LOOP else "int")
                except AssertionError as e:
                    _fail("ncc", g, i, k, p, f"form {form} (ran {ran}) costs", str(e))
                for what, want in (("the rule on the call's own costs", XM.ncc_wta(cost[p], win)), ("O.ncc", o["disp"])):
                    if disp[p].tobytes() != np.ascontiguousarray(want).tobytes():
                        _fail("ncc", g, i, k, p, f"form {form}: map against {what}", FC.first_diff(disp[p], want))


@pytest.mark.parametrize("g", _groups("asw"), ids=_gid)
def test_asw_chain(flows, O, g):
    """the flow's maps are the first-minimum rule on the costs smt_asw_both gives for the same pair, those costs are held
    to the exact reference, and the cross-checked map is O.asw_crosscheck of the flow's own two maps
    (tests/test_fuzz_flows_gpu.py)"""
    smt = flows
    ws, D, H, W = g["winSize"], g["D"], g["H"], g["W"]
    f = smt.ASWFlow(H, W, D, DEV, winSize=ws)

    def enqueue(f, t):
        return dict(zip(("dl", "dr", "last"), f.run(*t)))
    try:
        got = run_chain("asw", g, O, f, enqueue, lambda f: None)
    finally:
        f.close()
    sp, cm = smt.asw_masks(ws, FC.ASW_SIGMA_SPACE, FC.ASW_SIGMA_COLOR, DEV)
    for i, k in enumerate(SC.CHAIN[:-1]):                                        # the repeat equals position 0 byte for byte
        outs, _ = FC.oracle_batch("asw", g, k, O)
        for p, o in enumerate(outs):
            _, _, cl, cr = smt.AdaptiveSupportWeightBoth(T(o["Lp"]), T(o["Rp"]), ws, D, sp, cm, FC.ASW_T, want_cost=True)
            for v, cost, name in ((0, cl.cpu().numpy(), "dl"), (1, cr.cpu().numpy(), "dr")):
                try:
                    XM.check_asw(cost, o["exact_l" if v == 0 else "exact_r"], ws, XM.asw_nan_mask(H, W, D, ws, v))
                except AssertionError as e:
                    _fail("asw", g, i, k, p, f"view {v} costs", str(e))
                if got[i][name][p].tobytes() != XM.asw_wta(cost).tobytes():
                    _fail("asw", g, i, k, p, name, "differs from the first-minimum rule on the pair's own costs: " +
                          FC.first_diff(got[i][name][p], XM.asw_wta(cost)))
            want = O.asw_crosscheck(got[i]["dl"][p], got[i]["dr"][p])
            if got[i]["last"][p].tobytes() != np.ascontiguousarray(want).tobytes():
                _fail("asw", g, i, k, p, "lastDisp", FC.first_diff(got[i]["last"][p], want))
