"""The AdamW steps that also keep averaged weights (train.ema_decay) on the GPU:
mdemi_adamw_step_ema16 / mdemi_adamw_step_dev_ema16 (csrc/misc.hip).

Weights, moments, counters and bf16 copies are compared bit for bit with the same steps through
mdemi_adamw_step16 / mdemi_adamw_step_dev16: the EMA kernels are that body plus one more read
and write.  The averages are compared with an fp64 recurrence driven by the GPU's own post-step
weights, e64 <- e64 + (1 - d)(p_k - e64), under the bound

    |e - e64| <= 4 * 2^-24 * max_k max(|p_k|, |e_k|) / (1 - d)

per element: one fp32 rounding of the difference, one of the fma and one of 1 - d per step (three
half-ulps of the largest operand, rounded up to four), summed geometrically over the steps since
each step scales the error it inherits by d.  Under warm-up d varies per step; every d_k <= decay,
so the same sum is bounded with d = decay."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (numel, group, bf16 copy, average): a scalar-tail-only tensor, one shorter than two float4s,
# a float4 body without a tail, two chunks (65536 + 5: the second chunk is a scalar tail), one
# whose average is a view offset by one element (4-byte aligned only: scalar accesses to the
# average, while its weights must still come out as the plain step writes them), and one
# without an average (a null ema_dev entry)
SIZES = (1, 7, 4096, 65536 + 5, 1030, 515)
GROUP = (0, 0, 0, 1, 1, 1)
B16 = (2, 3, 4)
EMA_KIND = ("own", "own", "own", "own", "offset", None)
STEPS0 = (3, 0, 7, 2, 0, 5)  # per-parameter counts before the first step (tensor i uses slot i)
S0 = 2  # *step_dev before the first step
NSTEPS = 5
DECAY = 0.9
ROWS = [[(1e-3 * (s + 1), 0.9 - 0.01 * s, 0.999, 1e-8, 0.01), (2e-4 * (s + 1), 0.85 + 0.01 * s, 0.99, 1e-6, 0.1)]
        for s in range(S0 + NSTEPS + 1)]
MAX_NORM = 1.0  # the table's gradient norm is ~130: the clip is active when on
U = 2.0 ** -24


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Table:
    """One instance of the six-tensor problem on the device; every instance starts from the
    same values.  ``off`` is a seventh parameter with an average and no gradient: it is not in
    the table at all."""

    def __init__(self, updates0=0):
        from mdemi import _lib as L
        self.L, self.lib = L, L.load()
        g = torch.Generator().manual_seed(11)
        self.p = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
        self.m = [(torch.randn(n, generator=g) * 0.1).to(DEV) for n in SIZES]
        self.v = [(torch.rand(n, generator=g) * 0.01).to(DEV) for n in SIZES]
        self.g0 = [torch.randn(n, generator=g) * 0.5 for n in SIZES]  # the finite gradients (host)
        self.g = [t.to(DEV) for t in self.g0]
        self.p16 = {i: self.p[i].to(torch.bfloat16) for i in B16}
        # averages start away from the weights, so a wrong coefficient or operand shows at once
        self.e_store, self.e = [], []
        for n, kind in zip(SIZES, EMA_KIND):
            if kind is None:
                self.e_store.append(None)
                self.e.append(None)
                continue
            store = torch.randn(n + (1 if kind == "offset" else 0), generator=g).to(DEV)
            self.e_store.append(store)
            self.e.append(store[1:] if kind == "offset" else store)
        assert self.e[4].data_ptr() % 16 == 4 and all(self.e[i].data_ptr() % 16 == 0 for i in range(4))
        self.off_p = torch.randn(33, generator=g).to(DEV)
        self.off_e = torch.randn(33, generator=g).to(DEV)
        self.tsteps = torch.tensor(STEPS0, dtype=torch.int32).to(DEV)
        self.step_dev = torch.tensor([S0], dtype=torch.int32).to(DEV)
        self.guard = torch.tensor([0, 0, -1, 0], dtype=torch.int32).to(DEV)
        self.ema_state = torch.tensor([updates0], dtype=torch.int32).to(DEV)
        self.sumsq = torch.zeros(1, device=DEV)
        self.sched = torch.tensor([v for r in ROWS for e in r for v in (*e, 0.0)], dtype=torch.float32).to(DEV)
        chunk = self.lib.mdemi_multi_tensor_chunk()
        assert chunk == 65536
        refs = (L.TensorRef * len(SIZES))()
        items_t, items_c = [], []
        for i, n in enumerate(SIZES):
            r = refs[i]
            r.param, r.grad = self.p[i].data_ptr(), self.g[i].data_ptr()
            r.exp_avg, r.exp_avg_sq = self.m[i].data_ptr(), self.v[i].data_ptr()
            r.numel, r.group, r.step_slot = n, GROUP[i], i
            nch = max(1, math.ceil(n / chunk))
            items_t += [i] * nch
            items_c += list(range(nch))
        self.nt, self.ni = len(SIZES), len(items_t)
        assert self.ni == 7
        self.table = torch.frombuffer(bytearray(bytes(refs)), dtype=torch.uint8).to(DEV)
        ws = torch.zeros(self.lib.mdemi_grad_norm_workspace_size(self.ni) // 4, dtype=torch.int32)
        ws[:2 * self.ni] = torch.tensor(items_t + items_c, dtype=torch.int32)
        self.ws = ws.to(DEV)
        self.p16tab = torch.tensor([self.p16[i].data_ptr() if i in self.p16 else 0 for i in range(self.nt)],
                                   dtype=torch.int64).to(DEV)
        self.ematab = torch.tensor([e.data_ptr() if e is not None else 0 for e in self.e], dtype=torch.int64).to(DEV)

    def buffers(self):
        """Everything the AdamW arithmetic may write besides *step_dev and the guard state."""
        return [*self.p, *self.m, *self.v, *(self.p16[i] for i in B16), self.tsteps]

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone() for b in self.buffers()]

    def averages(self):
        """The averages' whole storage (the offset one with the element in front of the view),
        the off-table pair and the update count."""
        torch.cuda.synchronize()
        return [*(s.clone() for s in self.e_store if s is not None), self.off_p.clone(), self.off_e.clone(),
                self.ema_state.clone()]

    def set_grads(self, k=0, kind=None):
        for dst, src in zip(self.g, self.g0):
            dst.copy_(src * (1.0 + 0.25 * k))
        if kind == "nan_last":  # the last element of the table's two-chunk tensor
            self.g[3][-1] = float("nan")
        elif kind == "inf_scalar":  # the numel-1 tensor: scalar tail only
            self.g[0][0] = float("inf")
        elif kind == "overflow":  # finite, but its square is beyond fp32
            self.g[2][17] = 2e19
        else:
            assert kind is None

    def _groups(self, row):
        gr = (self.L.AdamWGroup * 2)()
        for i, e in enumerate(ROWS[row]):
            gr[i].lr, gr[i].beta1, gr[i].beta2, gr[i].eps, gr[i].weight_decay = e
        return gr

    def grad_sumsq(self):
        L = self.L
        L.check(self.lib.mdemi_grad_sumsq(self.table.data_ptr(), self.nt, self.ni, 1.0, self.sumsq.data_ptr(),
                                          self.ws.data_ptr(), L.stream()), "grad_sumsq")

    def step(self, form, clip, row=None, ema=True, guarded=False, decay=DECAY, warmup=False, ematab="own",
             state="own", sumsq="own"):
        """One update; returns the entry point's code.  ema=False: the existing unguarded entry
        point, which gets the sumsq pointer only with the clip on, as FusedAdamW passes it."""
        L, lib = self.L, self.lib
        max_norm = MAX_NORM if clip else 0.0
        sq = self.sumsq.data_ptr() if (sumsq == "own" and (clip or guarded)) else None
        tl, ws, p16, st = self.table.data_ptr(), self.ws.data_ptr(), self.p16tab.data_ptr(), L.stream()
        tail = (self.ematab.data_ptr() if ematab == "own" else None, decay, int(warmup),
                self.ema_state.data_ptr() if state == "own" else None, self.guard.data_ptr() if guarded else None)
        if form == "host":
            if ema:
                return lib.mdemi_adamw_step_ema16(tl, self.nt, self._groups(row), 2, sq, max_norm, 1.0, 1,
                                                  self.tsteps.data_ptr(), self.ni, p16, *tail, ws, st)
            return lib.mdemi_adamw_step16(tl, self.nt, self._groups(row), 2, sq, max_norm, 1.0, 1,
                                          self.tsteps.data_ptr(), self.ni, p16, ws, st)
        if ema:
            return lib.mdemi_adamw_step_dev_ema16(tl, self.nt, self.sched.data_ptr(), len(ROWS), 2,
                                                  self.step_dev.data_ptr(), self.tsteps.data_ptr(), sq, max_norm, 1.0,
                                                  self.ni, p16, *tail, ws, st)
        return lib.mdemi_adamw_step_dev16(tl, self.nt, self.sched.data_ptr(), len(ROWS), 2, self.step_dev.data_ptr(),
                                          self.tsteps.data_ptr(), sq, max_norm, 1.0, self.ni, p16, ws, st)


def _names():
    n = len(SIZES)
    return ([f"param{i}" for i in range(n)] + [f"exp_avg{i}" for i in range(n)] +
            [f"exp_avg_sq{i}" for i in range(n)] + [f"bf16_{i}" for i in B16] + ["tensor_steps"])


def _assert_same_buffers(a, b, what):
    for name, x, y in zip(_names(), a, b):
        assert _same(x, y), f"{what}: {name} differs"


def _assert_same_averages(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same(x, y), f"{what}: average buffer {i} differs"


def _d32(n, warmup):
    """The kernel's decay for update count n, in fp32."""
    d = np.float32(DECAY)
    if warmup:
        d = min(d, (np.float32(1) + np.float32(n)) / (np.float32(10) + np.float32(n)))
    return float(d)


def _run_five(form, clip, warmup, updates0):
    """Five EMA steps next to five plain ones; returns the EMA table, the per-step weights
    (index 0: before the first step) and averages, as fp64 arrays, of the averaged tensors."""
    t, ref = Table(updates0), Table()
    idx = [i for i, e in enumerate(t.e) if e is not None]
    ps = [[t.p[i].double().cpu().numpy() for i in idx]]
    es = [[t.e[i].double().cpu().numpy() for i in idx]]
    for k in range(NSTEPS):
        for tab, ema in ((t, True), (ref, False)):
            tab.set_grads(k)
            if clip:
                tab.grad_sumsq()
            assert tab.step(form, clip, row=S0 + k, ema=ema, warmup=warmup) == 0
        _assert_same_buffers(t.snapshot(), ref.snapshot(), f"step {k + 1}: EMA vs plain")
        ps.append([t.p[i].double().cpu().numpy() for i in idx])
        es.append([t.e[i].double().cpu().numpy() for i in idx])
    assert t.tsteps.tolist() == [s + NSTEPS for s in STEPS0]
    if form == "dev":
        assert t.step_dev.item() == ref.step_dev.item() == S0 + NSTEPS
    assert t.ema_state.item() == updates0 + NSTEPS  # one per applied call
    for i in B16:  # the copies are the cast of the new weights
        assert _same(t.p16[i], t.p[i].to(torch.bfloat16))
    return t, idx, ps, es


def _recurrence(ps, es, j, ds, which="right"):
    e = es[0][j].copy()
    for k, d in enumerate(ds):
        if which == "right":
            e = e + (1.0 - d) * (ps[k + 1][j] - e)
        elif which == "swapped":  # d and 1 - d exchanged
            e = e + d * (ps[k + 1][j] - e)
        else:  # the weights before the step
            e = e + (1.0 - d) * (ps[k][j] - e)
    return e


def _bound(ps, es, j):
    big = np.zeros_like(es[0][j])
    for k in range(len(ps)):
        big = np.maximum(big, np.maximum(np.abs(ps[k][j]), np.abs(es[k][j])))
    return 4.0 * U * big / (1.0 - float(np.float32(DECAY)))


FORMS = pytest.mark.parametrize("form", ["host", "dev"])
CLIP = pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])


@FORMS
@CLIP
def test_five_steps_match_the_plain_step_and_the_fp64_average(form, clip):
    before = Table().averages()
    t, idx, ps, es = _run_five(form, clip, warmup=False, updates0=0)
    ds = [_d32(n, False) for n in range(NSTEPS)]
    for j, i in enumerate(idx):
        bound = _bound(ps, es, j)
        got = es[-1][j]
        err = np.abs(got - _recurrence(ps, es, j, ds))
        print(f"tensor {i} ({SIZES[i]}): max err/bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), f"tensor {i}: average off by {np.max(err / bound):.2f} x the bound"
        # the bound tells a wrong average apart
        for which in ("swapped", "pre"):
            wrong = np.abs(got - _recurrence(ps, es, j, ds, which))
            print(f"    {which}: max err/bound {np.max(wrong / bound):.1f}")
            assert np.max(wrong / bound) > 1.0, f"tensor {i}: the bound does not exclude the {which} average"
    after = t.averages()
    # the element in front of the offset view, the off-table parameter and its average: untouched
    assert t.e_store[4][0].item() == Table().e_store[4][0].item()
    n_store = len([s for s in t.e_store if s is not None])
    for x, y in zip(after[n_store:n_store + 2], before[n_store:n_store + 2]):
        assert _same(x, y)
    # the tensor with a null ema_dev entry took the plain step (checked above) and owns no average
    assert t.e[5] is None


@FORMS
@pytest.mark.parametrize("updates0", [0, 78], ids=["n0", "n78"])
def test_warmup_follows_the_device_counter(form, updates0):
    """d = min(decay, (1 + n) / (10 + n)): n = 0.. ramps from 0.1; n = 78.. crosses into the
    constant decay at n = 80 ((1 + 80) / (10 + 80) = 0.9)."""
    t, idx, ps, es = _run_five(form, True, warmup=True, updates0=updates0)
    ds = [_d32(updates0 + k, True) for k in range(NSTEPS)]
    assert ds[0] < ds[1] and (updates0 == 0 or ds[-1] == float(np.float32(DECAY)))
    flat = [float(np.float32(DECAY))] * NSTEPS
    for j, i in enumerate(idx):
        bound = _bound(ps, es, j)
        err = np.abs(es[-1][j] - _recurrence(ps, es, j, ds))
        assert np.all(err <= bound), f"tensor {i}: average off by {np.max(err / bound):.2f} x the bound"
        # without the ramp, or with a counter that does not advance, the average is another one
        assert np.max(np.abs(es[-1][j] - _recurrence(ps, es, j, flat)) / bound) > 1.0
        assert np.max(np.abs(es[-1][j] - _recurrence(ps, es, j, [ds[0]] * NSTEPS)) / bound) > 1.0


@FORMS
@CLIP
@pytest.mark.parametrize("kind", ["nan_last", "inf_scalar", "overflow"])
def test_a_skipped_step_leaves_the_averages_and_the_next_one_counts(form, clip, kind):
    b = Table()
    before, avg_before = b.snapshot(), b.averages()
    b.set_grads(0, kind)
    b.grad_sumsq()
    assert b.step(form, clip, row=S0, guarded=True) == 0
    _assert_same_buffers(b.snapshot(), before, f"skipped step ({kind})")
    _assert_same_averages(b.averages(), avg_before, f"skipped step ({kind})")
    assert not math.isfinite(b.sumsq.item())
    last = S0 if form == "dev" else 0
    assert b.guard.tolist() == [1, 1, last, 1] and b.ema_state.item() == 0
    assert b.step_dev.item() == (S0 + 1 if form == "dev" else S0)
    # the next, finite step: the plain step with the next schedule row, and one average update
    b.set_grads(0)
    b.grad_sumsq()
    assert b.step(form, clip, row=S0 + 1, guarded=True) == 0
    a = Table()
    a.step_dev.fill_(S0 + 1)
    a.set_grads(0)
    a.grad_sumsq()
    assert a.step(form, clip, row=S0 + 1, ema=False) == 0
    _assert_same_buffers(b.snapshot(), a.snapshot(), f"step after the skip ({kind})")
    assert b.guard.tolist() == [1, 0, last, 2] and b.ema_state.item() == 1
    d = float(np.float32(DECAY))
    for i, e in enumerate(b.e):
        if e is None:
            continue
        e0 = a.e[i].double().cpu().numpy()  # a's averages never moved: the initial values
        p1 = b.p[i].double().cpu().numpy()
        want = e0 + (1.0 - d) * (p1 - e0)
        bound = 4.0 * U * np.maximum(np.abs(p1), np.abs(e0)) / (1.0 - d)
        assert np.all(np.abs(e.double().cpu().numpy() - want) <= bound), f"tensor {i}"


@FORMS
def test_bad_arguments_are_refused_and_nothing_is_launched(form):
    b = Table()
    b.grad_sumsq()
    before, avg_before = b.snapshot(), b.averages()
    bad = [dict(ematab=None), dict(state=None), dict(decay=1.0), dict(decay=-0.125), dict(decay=float("nan")),
           dict(guarded=True, sumsq=None)]
    for kw in bad:
        assert b.step(form, True, row=S0, **kw) < 0, kw
        assert b"ema" in b.lib.mdemi_last_error()
    _assert_same_buffers(b.snapshot(), before, "refused call")
    _assert_same_averages(b.averages(), avg_before, "refused call")
    assert b.guard.tolist() == [0, 0, -1, 0] and b.step_dev.item() == S0
    # decay 0 is allowed: the average becomes the new weights, e0 + (p - e0) in fp32
    e0 = [None if e is None else e.clone() for e in b.e]
    assert b.step(form, True, row=S0, decay=0.0) == 0
    torch.cuda.synchronize()
    for p, e, old in zip(b.p, b.e, e0):
        if e is not None:
            assert torch.all((e - p).abs() <= 4.0 * U * torch.maximum(p.abs(), old.abs()))
    assert b.ema_state.item() == 1
