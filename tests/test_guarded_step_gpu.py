"""The guarded AdamW step (train.nonfinite: "skip") on the GPU: mdemi_adamw_step_guarded16 /
mdemi_adamw_step_dev_guarded16 (csrc/misc.hip) against the unguarded entry points, bit for bit;
FusedAdamW(skip_nonfinite=True) in a captured graph; a Trainer that meets one non-finite step.

Every comparison is bit equality (int views): the guarded kernels are the unguarded body behind
one predicate, so there is no tolerance to choose."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the table: a scalar-tail-only tensor, a float4 body + 3-element tail, a short one, and two
# chunks (65536 + 5) last, so that the table's last (tensor, chunk) item ends the table
SIZES = (1, 4099, 1030, 65536 + 5)
B16 = (1, 2)  # tensors with a maintained bf16 copy (one with a scalar tail)
GROUP = (0, 0, 1, 1)  # the last two sit in a second parameter group
STEPS0 = (3, 0, 7, 2)  # per-parameter counts before the step (tensor i uses slot i)
S0 = 2  # *step_dev before the step
# schedule rows (lr, beta1, beta2, eps, weight_decay) x 2 groups
ROWS = [[(1e-3 * (s + 1), 0.9 - 0.01 * s, 0.999, 1e-8, 0.01), (2e-4 * (s + 1), 0.85 + 0.01 * s, 0.99, 1e-6, 0.1)]
        for s in range(6)]
MAX_NORM = 1.0  # the table's gradient norm is ~130: the clip is active when on


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Table:
    """One instance of the four-tensor problem on the device; every instance starts from the
    same values."""

    def __init__(self):
        from mdemi import _lib as L
        self.L, self.lib = L, L.load()
        g = torch.Generator().manual_seed(11)
        self.p = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
        self.m = [(torch.randn(n, generator=g) * 0.1).to(DEV) for n in SIZES]
        self.v = [(torch.rand(n, generator=g) * 0.01).to(DEV) for n in SIZES]
        self.g0 = [torch.randn(n, generator=g) * 0.5 for n in SIZES]  # the finite gradients (host)
        self.g = [t.to(DEV) for t in self.g0]
        self.p16 = {i: self.p[i].to(torch.bfloat16) for i in B16}
        self.tsteps = torch.tensor(STEPS0, dtype=torch.int32).to(DEV)
        self.step_dev = torch.tensor([S0], dtype=torch.int32).to(DEV)
        self.guard = torch.tensor([0, 0, -1, 0], dtype=torch.int32).to(DEV)
        self.sumsq = torch.zeros(1, device=DEV)
        self.sched = torch.tensor([v for r in ROWS for e in r for v in (*e, 0.0)], dtype=torch.float32).to(DEV)
        chunk = self.lib.mdemi_multi_tensor_chunk()
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
        assert self.ni == 5 and items_c[-1] == 1
        self.table = torch.frombuffer(bytearray(bytes(refs)), dtype=torch.uint8).to(DEV)
        ws = torch.zeros(self.lib.mdemi_grad_norm_workspace_size(self.ni) // 4, dtype=torch.int32)
        ws[:2 * self.ni] = torch.tensor(items_t + items_c, dtype=torch.int32)
        self.ws = ws.to(DEV)
        self.p16tab = torch.tensor([self.p16[i].data_ptr() if i in self.p16 else 0 for i in range(self.nt)],
                                   dtype=torch.int64).to(DEV)

    def buffers(self):
        """Everything an update may write besides *step_dev and the guard state."""
        return [*self.p, *self.m, *self.v, *(self.p16[i] for i in B16), self.tsteps]

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone() for b in self.buffers()]

    def set_grads(self, kind=None):
        for dst, src in zip(self.g, self.g0):
            dst.copy_(src)
        if kind == "nan_last":  # the last element of the table's last chunk
            self.g[3][-1] = float("nan")
        elif kind == "inf_scalar":  # the numel-1 tensor: scalar tail only
            self.g[0][0] = float("inf")
        elif kind == "overflow":  # finite, but its square is beyond fp32
            self.g[1][17] = 2e19
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

    def step(self, form, guarded, clip, row=None, sumsq="own"):
        """One update; returns the entry point's code.  form "host": hyperparameters of ROWS[row]
        by value; "dev": the device schedule at *step_dev.  The unguarded call gets the sumsq
        pointer only with the clip on, as FusedAdamW passes it."""
        L, lib = self.L, self.lib
        max_norm = MAX_NORM if clip else 0.0
        sq = self.sumsq.data_ptr() if sumsq == "own" else None
        tl, ws, p16, st = self.table.data_ptr(), self.ws.data_ptr(), self.p16tab.data_ptr(), L.stream()
        if form == "host":
            if guarded:
                return lib.mdemi_adamw_step_guarded16(tl, self.nt, self._groups(row), 2, sq, max_norm, 1.0,
                                                      self.tsteps.data_ptr(), self.ni, p16, self.guard.data_ptr(), ws,
                                                      st)
            return lib.mdemi_adamw_step16(tl, self.nt, self._groups(row), 2, sq if clip else None, max_norm, 1.0, 1,
                                          self.tsteps.data_ptr(), self.ni, p16, ws, st)
        if guarded:
            return lib.mdemi_adamw_step_dev_guarded16(tl, self.nt, self.sched.data_ptr(), len(ROWS), 2,
                                                      self.step_dev.data_ptr(), self.tsteps.data_ptr(), sq, max_norm,
                                                      1.0, self.ni, p16, self.guard.data_ptr(), ws, st)
        return lib.mdemi_adamw_step_dev16(tl, self.nt, self.sched.data_ptr(), len(ROWS), 2, self.step_dev.data_ptr(),
                                          self.tsteps.data_ptr(), sq if clip else None, max_norm, 1.0, self.ni, p16,
                                          ws, st)


def _assert_same_buffers(a, b, what):
    names = ([f"param{i}" for i in range(4)] + [f"exp_avg{i}" for i in range(4)] +
             [f"exp_avg_sq{i}" for i in range(4)] + [f"bf16_{i}" for i in B16] + ["tensor_steps"])
    for name, x, y in zip(names, a, b):
        assert _same(x, y), f"{what}: {name} differs"


FORMS = pytest.mark.parametrize("form", ["host", "dev"])
CLIP = pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])


@FORMS
@CLIP
def test_finite_gradients_guarded_equals_unguarded(form, clip):
    a, b = Table(), Table()
    before = a.snapshot()
    for t, guarded in ((a, False), (b, True)):
        t.grad_sumsq()
        assert t.step(form, guarded, clip, row=S0) == 0
    got, want = b.snapshot(), a.snapshot()
    _assert_same_buffers(got, want, "guarded vs unguarded")
    assert not _same(want[0], before[0]) and not _same(want[3], before[3])  # the step did something
    assert b.tsteps.tolist() == [s + 1 for s in STEPS0]
    for i in B16:  # the copies are the cast of the new weights
        assert _same(b.p16[i], b.p[i].to(torch.bfloat16))
    if form == "dev":
        assert a.step_dev.item() == b.step_dev.item() == S0 + 1
    assert b.guard.tolist() == [0, 0, -1, 1]
    assert a.guard.tolist() == [0, 0, -1, 0]


@FORMS
@CLIP
@pytest.mark.parametrize("kind", ["nan_last", "inf_scalar", "overflow"])
def test_nonfinite_gradients_are_skipped_then_the_next_step_applies(form, clip, kind):
    b = Table()
    before = b.snapshot()
    b.set_grads(kind)
    assert all(torch.isfinite(g).all() for g in b.g) == (kind == "overflow")
    b.grad_sumsq()
    assert b.step(form, True, clip, row=S0) == 0
    _assert_same_buffers(b.snapshot(), before, f"skipped step ({kind})")
    assert not math.isfinite(b.sumsq.item())
    assert b.tsteps.tolist() == list(STEPS0)
    last = S0 if form == "dev" else 0  # the schedule step, or the call count before the call
    assert b.guard.tolist() == [1, 1, last, 1]
    assert b.step_dev.item() == (S0 + 1 if form == "dev" else S0)  # the schedule position advanced
    # a finite step next: the unguarded step on the pre-skip state with the NEXT schedule row
    # and the un-advanced per-parameter counts
    b.set_grads(None)
    b.grad_sumsq()
    assert b.step(form, True, clip, row=S0 + 1) == 0
    a = Table()
    a.step_dev.fill_(S0 + 1)
    a.grad_sumsq()
    assert a.step(form, False, clip, row=S0 + 1) == 0
    _assert_same_buffers(b.snapshot(), a.snapshot(), f"step after the skip ({kind})")
    assert b.tsteps.tolist() == [s + 1 for s in STEPS0]
    if form == "dev":
        assert a.step_dev.item() == b.step_dev.item() == S0 + 2
    assert b.guard.tolist() == [1, 0, last, 2]
    # and it is not what row S0 would have given (the schedule did move)
    c = Table()
    c.grad_sumsq()
    assert c.step(form, False, clip, row=S0) == 0
    assert not _same(c.snapshot()[1], b.snapshot()[1])


@FORMS
def test_missing_sumsq_is_an_error_and_nothing_is_launched(form):
    b = Table()
    before = b.snapshot()
    for clip in (False, True):
        rc = b.step(form, True, clip, row=S0, sumsq=None)
        assert rc < 0
        msg = b.lib.mdemi_last_error()
        assert b"guarded" in msg and b"sumsq" in msg, msg
    _assert_same_buffers(b.snapshot(), before, "refused call")
    assert b.guard.tolist() == [0, 0, -1, 0] and b.step_dev.item() == S0
    # the other required pointers
    L, lib = b.L, b.lib
    assert lib.mdemi_adamw_step_guarded16(b.table.data_ptr(), b.nt, b._groups(0), 2, b.sumsq.data_ptr(), 0.0, 1.0,
                                          b.tsteps.data_ptr(), b.ni, None, None, b.ws.data_ptr(), L.stream()) < 0
    assert lib.mdemi_adamw_step_dev_guarded16(b.table.data_ptr(), b.nt, b.sched.data_ptr(), len(ROWS), 2,
                                              b.step_dev.data_ptr(), None, b.sumsq.data_ptr(), 0.0, 1.0, b.ni, None,
                                              b.guard.data_ptr(), b.ws.data_ptr(), L.stream()) < 0
    _assert_same_buffers(b.snapshot(), before, "refused call")


# ---------------------------------------------------------------- FusedAdamW in a captured graph
def _opt_params():
    g = torch.Generator().manual_seed(5)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in (1, 4099, 65536 + 5)]


def _fused(ps, rows, **kw):
    from mdemi.train import FusedAdamW
    opt = FusedAdamW([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3, max_grad_norm=MAX_NORM, capturable=True, **kw)
    opt.set_schedule(rows)
    return opt


def test_captured_graph_skips_on_replay():
    g = torch.Generator().manual_seed(6)
    grads = [[(torch.randn(n, generator=g) * 0.5).to(DEV) for n in (1, 4099, 65536 + 5)] for _ in range(3)]
    grads[1][2][-1] = float("nan")
    rows = [r for r in ROWS[:4]]
    ps = _opt_params()
    init = [p.detach().clone() for p in ps]
    opt = _fused(ps, rows, skip_nonfinite=True)
    static = [torch.zeros_like(p) for p in ps]
    for p, s in zip(ps, static):
        p.grad = s
    # one eager step allocates the counters, the guard state and the schedule (none may be
    # created inside a capture); then everything goes back to step 0
    for s, gr in zip(static, grads[0]):
        s.copy_(gr)
    opt.step()
    assert opt.skipped_steps() == (0, 0)
    sd = opt.state_dict()
    assert sd["schedule_step"] == 1
    zero = {"state": {i: {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(v["exp_avg"]),
                          "exp_avg_sq": torch.zeros_like(v["exp_avg_sq"])} for i, v in sd["state"].items()},
            "param_groups": sd["param_groups"], "schedule_step": 0}
    opt.load_state_dict(zero)
    with torch.no_grad():
        for p, p0 in zip(ps, init):
            p.copy_(p0)
    assert opt.step_count == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(3):  # finite / NaN / finite
        for s, gr in zip(static, grads[k]):
            s.copy_(gr)
        graph.replay()
        opt.replayed()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == (1, 0)
    assert opt.step_count == 3 and opt.steps == [2, 2, 2]
    assert opt._guard_dev.tolist()[2] == 1  # the schedule step that was dropped
    # reference: the unguarded optimizer, eager, steps 1 and 3 under schedule rows 0 and 2
    qs = _opt_params()
    ref = _fused(qs, [rows[0], rows[2]])
    for k in (0, 2):
        for q, gr in zip(qs, grads[k]):
            q.grad = gr.clone()
        ref.step()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert _same(p.detach(), q.detach()), f"param {i}"
        for k in ("exp_avg", "exp_avg_sq"):
            assert _same(opt.state[p][k], ref.state[q][k]), f"{k} {i}"
    sd = opt.state_dict()
    assert sd["schedule_step"] == 3 and [float(v["step"]) for v in sd["state"].values()] == [2.0, 2.0, 2.0]


# ---------------------------------------------------------------- Trainer (tiny07, 64x96, batch 2)
def _data(n, bad=None):
    g = torch.Generator().manual_seed(3)
    out = [(torch.randn(2, 3, 64, 96, generator=g).to(DEV), (torch.rand(2, 1, 64, 96, generator=g) * 9 + 0.5).to(DEV))
           for _ in range(n)]
    if bad is not None:  # one ground-truth pixel +inf: it passes SILog's gt > min_depth mask
        out[bad][1][1, 0, 17, 23] = float("inf")
    return out


def _trainer(telemetry, graph=False, skip=True):
    from mdemi.model.NewCRFs import NewCRFDepth
    from mdemi.train import FusedAdamW, OneCycleLR, SILogLoss
    from mdemi.train.builder import Trainer
    torch.manual_seed(0)
    m = NewCRFDepth(version="tiny07", max_depth=10.0, drop_path_rate=0.0).to(DEV).train()
    kw = {"skip_nonfinite": True} if skip else {}
    opt = FusedAdamW(m.parameters(), lr=2e-4, weight_decay=0.01, max_grad_norm=0.1, capturable=graph, **kw)
    sched = OneCycleLR(opt, max_lr=2e-4, total_steps=10, pct_start=0.3)
    return Trainer({"train": {}}, m, SILogLoss(10.0, 0.15), opt, sched, graph=graph, telemetry=telemetry)


def _state(t):
    torch.cuda.synchronize()
    out = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    for i, p in enumerate(t.model.parameters()):
        st = t.optimizer.state.get(p)
        if st is not None:
            out[f"exp_avg.{i}"] = st["exp_avg"].clone()
            out[f"exp_avg_sq.{i}"] = st["exp_avg_sq"].clone()
    return out


def _equal_states(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_survives_one_nonfinite_step_and_resumes_bit_equal(graph, tmp_path):
    from mdemi import _lib as L
    from mdemi.train.telemetry import Telemetry
    data = _data(6, bad=2)
    tel = Telemetry(capacity=8)
    t = _trainer(tel, graph=graph)
    states = []
    for b in data[:5]:
        t.step([b])
        states.append(_state(t))
    assert all(torch.isfinite(v).all() for v in states[2].values() if v.is_floating_point())  # the forward too
    # the batch statistics of step 3's (finite) forward did reach the BatchNorm buffers; the
    # weights and moments stood still
    moved = _equal_states(states[1], states[2])
    assert all("running_" in k or "num_batches_tracked" in k for k in moved), moved
    params = {k for k, _ in t.model.named_parameters()}
    for a, b in ((0, 1), (2, 3), (3, 4)):
        assert params & set(_equal_states(states[a], states[b])), f"step {b + 1} changed no weight"
    assert all(torch.isfinite(v).all() for v in states[4].values() if v.is_floating_point())
    d = tel.drain(raise_on_nonfinite=False)
    assert [r.index for r in d.records] == [0, 1, 2, 3, 4]
    assert [r.index for r in d.records if r.flags] == [2]
    assert d.records[2].flags & L.STEP_GRAD_NONFINITE
    assert t.optimizer.skipped_steps() == (1, 0)
    assert t.optimizer.step_count == 5 and set(t.optimizer.steps) == {4}
    # checkpoint after step 5, then the sixth step straight and resumed
    t.epoch = 0
    t.save("five", str(tmp_path), 5, 0.5)
    t.step([data[5]])
    want = _state(t)
    t.save("six", str(tmp_path), 6, 0.5)
    for name, per_param, sched_step in (("five", 4.0, 5), ("six", 5.0, 6)):
        osd = torch.load(tmp_path / f"{name}.pth", map_location="cpu", weights_only=True)["optimizer_state_dict"]
        assert osd["schedule_step"] == sched_step
        assert {float(v["step"]) for v in osd["state"].values()} == {per_param}
    t2 = _trainer(Telemetry(capacity=8), graph=graph)
    t2.resume(str(tmp_path / "five.pth"))
    assert t2.optimizer.step_count == 5 and t2.scheduler.last_step == 5
    t2.step([data[5]])
    got = _state(t2)
    assert _equal_states(want, got) == []
    assert t2.optimizer.state_dict()["schedule_step"] == 6


def test_fit_runs_through_a_skipped_step_with_the_real_trainer(tmp_path):
    """The driver loop on the real Trainer, Telemetry and guard state: the records and
    FusedAdamW.skipped_steps() agree at every drain (fit raises if they do not)."""
    import json
    from mdemi.train.loop import fit
    from mdemi.train.telemetry import Telemetry
    data = _data(6, bad=2)
    t = _trainer(Telemetry(capacity=8))
    opt = {"dataloader": {"batch_size": 2},
           "train": {"print_freq": 2, "valid_freq": 100, "epoch": 1, "num_accum": 1, "nonfinite": "skip"}}
    code = fit(t, iter([[b] for b in data]), lambda: {"abs_rel": 0.5}, opt, str(tmp_path), steps_per_epoch=6,
               log=lambda s: None)
    assert code == 0
    log = [json.loads(s) for s in open(tmp_path / "log.jsonl")]
    assert [r for r in log if r["type"] == "skipped"] == [{"type": "skipped", "step": 3, "epoch": 0, "iter": 3}]
    train = [r for r in log if r["type"] == "train"]
    assert [(r["step"], r["skipped"], r["skipped_total"]) for r in train] == [(2, 0, 0), (4, 1, 1), (6, 0, 1)]
    assert all(math.isfinite(r["loss"]) and math.isfinite(r["grad_norm"]) and math.isfinite(r["param_norm"])
               for r in train)
    assert [r["step"] for r in log if r["type"] == "valid"] == [6]
    osd = torch.load(tmp_path / "latest.pth", map_location="cpu", weights_only=True)["optimizer_state_dict"]
    assert osd["schedule_step"] == 6 and {float(v["step"]) for v in osd["state"].values()} == {5.0}
    # the same loop without the guarded optimizer refuses to call anything "skipped"
    with pytest.raises(ValueError, match="skip_nonfinite"):
        fit(_trainer(Telemetry(capacity=8), skip=False), iter([]), lambda: {}, opt, str(tmp_path), steps_per_epoch=6)


def test_default_policy_still_raises_on_the_same_data():
    from mdemi.train.telemetry import NonFiniteStep, Telemetry
    data = _data(3, bad=2)
    tel = Telemetry(capacity=8)
    t = _trainer(tel, skip=False)
    for b in data:
        t.step([b])
    with pytest.raises(NonFiniteStep) as e:
        tel.drain()
    assert e.value.first_index == 2 and e.value.count == 1
    assert t.optimizer.skip_nonfinite is False and "schedule_step" not in t.optimizer.state_dict()
