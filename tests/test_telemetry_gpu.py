"""Step telemetry on the GPU: mdemi_param_sumsq, mdemi_telemetry_push (csrc/telemetry.hip),
FusedAdamW.grad_sumsq_tensor / param_norm and the Trainer hook."""
import ctypes
import math
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# one table whose (tensor, chunk) items cross tensors: sizes around the 65536-element chunk and
# the float4 body / scalar tail split, plus a 4-byte-aligned slice (the scalar path)
SIZES = (1, 3, 4, 255, 65535, 65536, 65537, 2 * 65536 + 5)
SLICE = 70001
SEED = 20260
# mdemi_grad_sumsq over this table's gradients (SEED above, grad_scale 1) as the parent commit's
# libmdemi.so (f407298, before csrc/telemetry.hip existed) computed it on an MI355X: the float32
# bits of 99499.34375 (fp64 sum 99499.34698631453).  The existing kernels must not move.
PARENT_GRAD_SUMSQ_BITS = 0x47C255AC


def build_table(lib_mod, seed=SEED):
    """(params, grads, table, workspace, ntensors, nitems) on the device."""
    L = lib_mod
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
    grads = [(torch.randn(n, generator=g) * 0.5).to(DEV) for n in SIZES]
    pbuf = torch.randn(SLICE + 1, generator=g).to(DEV)
    gbuf = (torch.randn(SLICE + 1, generator=g) * 0.5).to(DEV)
    params.append(pbuf[1:])
    grads.append(gbuf[1:])
    assert params[-1].is_contiguous() and params[-1].data_ptr() % 16 == 4
    chunk = L.load().mdemi_multi_tensor_chunk()
    refs = (L.TensorRef * len(params))()
    items_t, items_c = [], []
    for ti, (p, gr) in enumerate(zip(params, grads)):
        refs[ti].param, refs[ti].grad, refs[ti].numel = p.data_ptr(), gr.data_ptr(), p.numel()
        nch = max(1, math.ceil(p.numel() / chunk))
        items_t += [ti] * nch
        items_c += list(range(nch))
    ni = len(items_t)
    table = torch.frombuffer(bytearray(bytes(refs)), dtype=torch.uint8).to(DEV)
    ws = torch.zeros(L.load().mdemi_grad_norm_workspace_size(ni) // 4, dtype=torch.int32)
    ws[:2 * ni] = torch.tensor(items_t + items_c, dtype=torch.int32)
    return params, grads, table, ws.to(DEV), len(params), ni


def grad_sumsq_bits(lib_mod):
    L = lib_mod
    _, grads, table, ws, nt, ni = build_table(L)
    out = torch.zeros(1, device=DEV)
    L.check(L.load().mdemi_grad_sumsq(table.data_ptr(), nt, ni, 1.0, out.data_ptr(), ws.data_ptr(), L.stream()),
            "grad_sumsq")
    torch.cuda.synchronize()
    return struct.unpack("<I", struct.pack("<f", out.item()))[0], grads


def test_param_sumsq_against_fp64():
    """Bar 2e-5 relative, from the summation depth: every term is non-negative and at most
    OPT_CHUNK / OPT_THREADS + log2(OPT_THREADS) + 4 = 268 fp32 roundings touch any value (256
    fused multiply-adds per thread, the stream / wave / block sums, the fp32 store of the fp64
    final), so the relative error is at most 268 * 2^-24 ~ 1.6e-5.  The kernel sums as
    sumsq_partial / sumsq_final do."""
    from mdemi import _lib as L
    params, _, table, ws, nt, ni = build_table(L)
    assert ni > nt  # multi-chunk tensors
    out = torch.zeros(1, device=DEV)
    L.check(L.load().mdemi_param_sumsq(table.data_ptr(), nt, ni, out.data_ptr(), ws.data_ptr(), L.stream()),
            "param_sumsq")
    ref = sum(float(p.double().pow(2).sum()) for p in params)
    got = float(out.item())
    rel = abs(got - ref) / ref
    print(f"param_sumsq {got!r} vs fp64 {ref!r}: rel {rel:.3e}")
    assert rel <= 2e-5
    # deterministic: the same bits again
    out2 = torch.zeros(1, device=DEV)
    L.check(L.load().mdemi_param_sumsq(table.data_ptr(), nt, ni, out2.data_ptr(), ws.data_ptr(), L.stream()),
            "param_sumsq")
    assert torch.equal(out, out2)
    # argument checks
    lib = L.load()
    assert lib.mdemi_param_sumsq(None, nt, ni, out.data_ptr(), ws.data_ptr(), None) < 0
    assert lib.mdemi_param_sumsq(table.data_ptr(), nt, 0, out.data_ptr(), ws.data_ptr(), None) < 0
    assert b"param_sumsq" in lib.mdemi_last_error()


def test_grad_sumsq_unchanged_from_parent():
    from mdemi import _lib as L
    bits, grads = grad_sumsq_bits(L)
    ref = sum(float(g.double().pow(2).sum()) for g in grads)
    got = struct.unpack("<f", struct.pack("<I", bits))[0]
    print(f"grad_sumsq bits 0x{bits:08X} = {got!r} (fp64 {ref!r})")
    assert abs(got - ref) / ref <= 2e-5
    assert bits == PARENT_GRAD_SUMSQ_BITS, f"0x{bits:08X}"


def test_compute_param_norm_runs_on_param_sumsq():
    from mdemi import _lib as L
    from mdemi.utils.common_utils import compute_param_norm
    params, _, _, _, _, _ = build_table(L)
    ps = [p.clone().requires_grad_(True) for p in params[:-1]] + [params[-1].requires_grad_(True)]
    frozen = torch.randn(5, device=DEV)
    got = compute_param_norm(ps + [frozen])
    want = math.sqrt(sum(float(p.detach().double().pow(2).sum()) for p in ps))
    assert got.is_cuda and abs(got.item() - want) / want <= 2e-5
    # other norms and strided parameters take the torch path
    strided = torch.randn(8, 6, device=DEV).t().requires_grad_(True)
    assert compute_param_norm([strided]).item() == pytest.approx(strided.detach().norm().item(), rel=1e-6)
    assert compute_param_norm(ps[:3], 1.0).item() == pytest.approx(
        sum(p.detach().abs().sum().item() for p in ps[:3]), rel=1e-5)


def _push(L, tel, loss, gsq):
    lt = torch.tensor(loss, device=DEV, dtype=torch.float32)
    gt = None if gsq is None else torch.tensor(gsq, device=DEV, dtype=torch.float32)
    L.check(L.load().mdemi_telemetry_push(tel.ring_ptr, tel.capacity, tel.state_ptr, lt.data_ptr(), L.ptr(gt),
                                          L.stream()), "telemetry_push")
    torch.cuda.synchronize()


def test_telemetry_push_ring_flags_and_counters():
    from mdemi import _lib as L
    from mdemi.train.telemetry import NonFiniteStep, Telemetry
    tel = Telemetry(capacity=4, device=torch.device(DEV, 0))
    state, ring = tel.snapshot()
    assert state == {"pushed": 0, "nonfinite_steps": 0, "first_nonfinite": -1}
    losses = [1.0, 2.0, float("nan"), 4.0, 5.0, 6.0]  # push 3 (index 2): NaN loss
    gsqs = [0.25, None, 0.5, 0.75, float("inf"), 1.5]  # push 2: no gradient norm; push 5: inf
    for lo, gs in zip(losses, gsqs):
        _push(L, tel, lo, gs)
    state, ring = tel.snapshot()
    assert state == {"pushed": 6, "nonfinite_steps": 2, "first_nonfinite": 2}
    assert [int(r["index"]) for r in ring] == [4, 5, 2, 3]  # index i lives in slot i % 4
    by_index = {int(r["index"]): r for r in ring}
    assert [int(by_index[i]["flags"]) for i in (2, 3, 4, 5)] == [L.STEP_LOSS_NONFINITE, 0, L.STEP_GRAD_NONFINITE, 0]
    assert math.isnan(float(by_index[2]["loss"])) and float(by_index[2]["grad_sumsq"]) == 0.5
    assert [float(by_index[i]["loss"]) for i in (3, 4, 5)] == [4.0, 5.0, 6.0]
    assert math.isinf(float(by_index[4]["grad_sumsq"])) and float(by_index[5]["grad_sumsq"]) == 1.5
    with pytest.raises(NonFiniteStep) as e:
        tel.drain()
    assert e.value.first_index == 2 and e.value.count == 2
    # a null gradient norm is recorded as -1 with no gradient flag
    tel2 = Telemetry(capacity=4, device=torch.device(DEV, 0))
    _push(L, tel2, 7.0, None)
    d = tel2.drain()
    assert d.dropped == 0 and d.pushed == 1
    assert [tuple(r) for r in d.records] == [(7.0, -1.0, 0, 0)]
    assert tel2.drain().records == []
    for i in range(6):
        _push(L, tel2, float(i), 1.0)
    d = tel2.drain()
    assert [r.index for r in d.records] == [3, 4, 5, 6] and d.dropped == 2
    # argument checks
    lib = L.load()
    one = torch.zeros(1, device=DEV)
    assert lib.mdemi_telemetry_push(tel.ring_ptr, 0, tel.state_ptr, one.data_ptr(), None, None) < 0
    assert lib.mdemi_telemetry_push(None, 4, tel.state_ptr, one.data_ptr(), None, None) < 0
    assert lib.mdemi_telemetry_push(tel.ring_ptr, 4, None, one.data_ptr(), None, None) < 0
    assert lib.mdemi_telemetry_push(tel.ring_ptr, 4, tel.state_ptr, None, None, None) < 0
    assert b"telemetry_push" in lib.mdemi_last_error()


def test_telemetry_push_in_a_captured_graph_advances_per_replay():
    from mdemi.train.telemetry import Telemetry
    tel = Telemetry(capacity=4, device=torch.device(DEV, 0))
    loss = torch.tensor(1.5, device=DEV)
    tel.push(loss)
    torch.cuda.synchronize()
    before = tel.snapshot()[0]["pushed"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tel.push(loss)
    assert tel.snapshot()[0]["pushed"] == before  # a capture records, it does not run
    for k in range(3):
        loss.fill_(10.0 + k)
        g.replay()
    torch.cuda.synchronize()
    d = tel.drain()
    assert d.pushed == before + 3
    assert [(r.index, r.loss, r.grad_sumsq) for r in d.records] == [(0, 1.5, -1.0), (1, 10.0, -1.0), (2, 11.0, -1.0),
                                                                    (3, 12.0, -1.0)]


# ---------------------------------------------------------------- Trainer (tiny07, 64x96, batch 2)
def _data(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(2, 3, 64, 96, generator=g).to(DEV), (torch.rand(2, 1, 64, 96, generator=g) * 9 + 0.5).to(DEV))
            for _ in range(n)]


def _trainer(telemetry, graph=False, max_grad_norm=0.1):
    from mdemi.model.NewCRFs import NewCRFDepth
    from mdemi.train import FusedAdamW, OneCycleLR, SILogLoss
    from mdemi.train.builder import Trainer
    torch.manual_seed(0)
    m = NewCRFDepth(version="tiny07", max_depth=10.0, drop_path_rate=0.0).to(DEV).train()
    opt = FusedAdamW(m.parameters(), lr=2e-4, weight_decay=0.01, max_grad_norm=max_grad_norm, capturable=graph)
    sched = OneCycleLR(opt, max_lr=2e-4, total_steps=10, pct_start=0.3)
    return Trainer({"train": {}}, m, SILogLoss(10.0, 0.15), opt, sched, graph=graph, telemetry=telemetry)


def test_trainer_eager_records_match_and_leave_the_weights_alone():
    from mdemi.train.telemetry import Telemetry
    data = _data(4)
    tel = Telemetry(capacity=8)
    a = _trainer(tel)
    losses, sumsqs = [], []
    for b in data:
        losses.append(a.step([b]).clone())
        sumsqs.append(a.optimizer._sumsq.clone())
    d = tel.drain()
    assert d.dropped == 0 and [r.index for r in d.records] == [0, 1, 2, 3]
    for r, lo, sq in zip(d.records, losses, sumsqs):
        assert r.flags == 0
        assert r.loss == lo.item() and r.grad_sumsq == sq.item()  # fp32 -> float is exact: bit equality
    pn = a.optimizer.param_norm()
    # the table holds the parameters that had a gradient: the ones with optimizer state
    want = math.sqrt(sum(float(p.detach().double().pow(2).sum()) for p in a.optimizer.state))
    assert abs(pn.item() - want) / want <= 2e-5
    b = _trainer(None)
    for bt in data:
        b.step([bt])
    torch.cuda.synchronize()
    for (k, pa), pb in zip(a.model.state_dict().items(), b.model.state_dict().values()):
        assert torch.equal(pa, pb), k


def test_trainer_graph_mode_records_every_call():
    from mdemi.train.telemetry import Telemetry
    data = _data(5)
    tel = Telemetry(capacity=8)
    t = _trainer(tel, graph=True)
    losses = [t.step([b]).item() for b in data]  # 2 eager calls, the capture's replay, 2 replays
    d = tel.drain()
    assert d.pushed == 5 and [r.index for r in d.records] == [0, 1, 2, 3, 4]
    assert [r.loss for r in d.records] == losses
    assert all(r.flags == 0 and r.grad_sumsq > 0 for r in d.records)
    # the parameter norm between replays reads the captured step's table and leaves it usable
    pn = t.optimizer.param_norm().item()
    want = math.sqrt(sum(float(p.detach().double().pow(2).sum()) for p in t.optimizer.state))
    assert abs(pn - want) / want <= 2e-5
    loss6 = t.step([data[0]]).item()
    d = tel.drain()
    assert [(r.index, r.loss) for r in d.records] == [(5, loss6)] and d.records[0].grad_sumsq > 0


def test_trainer_without_clip_still_records_the_gradient_norm():
    from mdemi.train.telemetry import Telemetry
    data = _data(1)
    tel = Telemetry(capacity=4)
    t = _trainer(tel, max_grad_norm=0.0)
    t._zero_grad = lambda: None  # keep the step's gradients for the fp64 reference
    t.step([data[0]])
    rec = tel.drain().records[0]
    want = sum(float(p.grad.double().pow(2).sum()) for p in t.model.parameters() if p.grad is not None)
    print(f"grad_sumsq recorded {rec.grad_sumsq!r} vs fp64 over the gradients {want!r}")
    assert want > 0 and abs(rec.grad_sumsq - want) / want <= 2e-5
    assert rec.grad_sumsq == t.optimizer._sumsq.item()
