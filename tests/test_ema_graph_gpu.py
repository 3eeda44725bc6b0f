"""FusedAdamW with averaged weights (set_ema) inside a captured graph: the schedule, the
warm-up count and the averages all live on the device, so three replays must leave exactly
what three eager steps leave."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 4099, 65536 + 5, 33)  # the last parameter never gets a gradient
DECAY = 0.9


def _bits(t):
    return t.view(torch.int32)


def _build():
    from mdemi.train import FusedAdamW, OneCycleLR
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in SIZES]
    es = [torch.randn(n, generator=g).to(DEV) for n in SIZES]  # averages that start away from the weights
    opt = FusedAdamW([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3, weight_decay=0.01, max_grad_norm=1.0,
                     capturable=True)
    sched = OneCycleLR(opt, max_lr=1e-3, total_steps=10, pct_start=0.3)
    opt.set_schedule(sched.hyper_table())
    version = opt.layout_version
    opt.set_ema(dict(zip(ps, es)), DECAY, warmup=True)
    assert opt.layout_version > version  # a captured step would re-capture
    return ps, es, opt


def _grads():
    g = torch.Generator().manual_seed(6)
    return [[(torch.randn(n, generator=g) * 0.5).to(DEV) for n in SIZES[:3]] for _ in range(3)]


def test_set_ema_rejects_what_the_kernel_cannot_take():
    ps, es, opt = _build()
    with pytest.raises(ValueError, match="decay"):
        opt.set_ema({ps[0]: es[0]}, 1.0)
    with pytest.raises(ValueError, match="shape"):
        opt.set_ema({ps[0]: es[1]}, 0.5)
    with pytest.raises(ValueError, match="not a parameter"):
        opt.set_ema({torch.nn.Parameter(torch.zeros(3, device=DEV)): torch.zeros(3, device=DEV)}, 0.5)


def test_three_replays_equal_three_eager_steps():
    grads = _grads()
    # eager
    qs, fs, ref = _build()
    for k in range(3):
        for q, gr in zip(qs, grads[k]):
            q.grad = gr.clone()
        ref.step()
    torch.cuda.synchronize()
    assert ref.ema_updates() == 3
    # captured: one eager step creates the counters, the EMA state and the schedule (none may be
    # created inside a capture); then everything goes back to step 0
    ps, es, opt = _build()
    init_p = [p.detach().clone() for p in ps]
    init_e = [e.clone() for e in es]
    static = [torch.zeros_like(p) for p in ps[:3]]
    for p, s in zip(ps, static):
        p.grad = s
    for s, gr in zip(static, grads[0]):
        s.copy_(gr)
    opt.step()
    assert opt.ema_updates() == 1
    sd = opt.state_dict()
    zero = {"state": {i: {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(v["exp_avg"]),
                          "exp_avg_sq": torch.zeros_like(v["exp_avg_sq"])} for i, v in sd["state"].items()},
            "param_groups": sd["param_groups"]}
    opt.load_state_dict(zero)
    opt.set_ema_updates(0)
    with torch.no_grad():
        for p, p0 in zip(ps, init_p):
            p.copy_(p0)
        for e, e0 in zip(es, init_e):
            e.copy_(e0)
    assert opt.step_count == 0 and opt.ema_updates() == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(3):
        for s, gr in zip(static, grads[k]):
            s.copy_(gr)
        graph.replay()
        opt.replayed()
    torch.cuda.synchronize()
    assert opt.ema_updates() == 3 and opt.step_count == 3
    for i, (p, q, e, f) in enumerate(zip(ps, qs, es, fs)):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), f"param {i}"
        assert torch.equal(_bits(e), _bits(f)), f"average {i}"
    for i, (p, q) in enumerate(zip(ps[:3], qs[:3])):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(opt.state[p][k]), _bits(ref.state[q][k])), f"{k} {i}"
    # the averages did move, under the ramp (d = 0.1, 2/11, 3/12 -- far from the constant 0.9),
    # and the parameter without a gradient kept its weights and its average
    assert not torch.equal(es[1], init_e[1])
    d_ramp = (es[1] - init_e[1]).abs().max().item()
    assert d_ramp > 0.5 * (ps[1].detach() - init_e[1]).abs().max().item()
    assert torch.equal(_bits(es[3]), _bits(init_e[3])) and torch.equal(_bits(ps[3].detach()), _bits(init_p[3]))
