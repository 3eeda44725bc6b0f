"""The normalisation entry points of include/mdemi.h (csrc/layernorm.hip, csrc/chnorm.hip) against
the fp64 reference of tests/norm_contract_ref.py, through the C ABI itself (ctypes), so null
pointers, aliasing, alignment and entry points vary on their own.

Every call works on views into larger allocations the test owns (norm_contract_cases.Arena): NaN
around the inputs, a quiet-NaN pattern in the outputs and around them, a workspace of exactly
*_workspace_size bytes of NaN between two pattern guards.  After a call
  * every output it was given meets the per-block criterion of norm_contract_cases.check
    (tolerances: 4 x the error of the reference's own fp32 restatement, not measured on a kernel)
    and holds no NaN: it was written in full, from nothing but its inputs;
  * every slack word and every workspace guard still holds the pattern;
  * every output it was not given, and every output of a call that returned an error, is
    untouched bit for bit;
  * a bf16 copy is bit for bit the RNE rounding of the fp32 output the same call wrote.
Each check prints its worst normalised error before it asserts (pytest -s shows them)."""
import functools
from types import SimpleNamespace

import pytest
import torch

import norm_contract_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL, EWORKSPACE = -1, -4
GUARD64 = -99


@pytest.fixture(scope="module")
def L():
    from mdemi import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=2)
def prepared(case):
    """The case's allocations on the device (outputs pristine: cloned per Run) and its reference,
    computed once on the CPU in fp64."""
    problem, arena = {G.LNCase: (G.ln_problem, G.ln_arena), G.BNCase: (G.bn_problem, G.bn_arena),
                      G.GNCase: (G.gn_problem, G.gn_arena)}[type(case)]
    p = problem(case)
    a = arena(p)
    return SimpleNamespace(case=case, p=p, a=a, bufs0={n: t.to(DEV) for n, t in a.bufs.items()},
                           masks={n: m.to(DEV) for n, m in a.masks.items() if a.is_out[n]}, dev={})


class Run:
    """Calls on one fresh set of output allocations."""

    def __init__(self, L, case):
        self.L, self.lib, self.pr = L, L.load(), prepared(case)
        self.a, self.p, self.what = self.pr.a, self.pr.p, case.name
        self.bufs = {n: (t.clone() if self.a.is_out[n] else t) for n, t in self.pr.bufs0.items()}
        self.spaces = []
        self.tracked = torch.full((8,), GUARD64, dtype=torch.int64, device=DEV)
        self.tracked[3] = G.TRACKED0

    def ptr(self, name, extra=0):
        return None if name is None else self.bufs[name].data_ptr() + self.a.ptr_offset[name] + extra

    def tracked_ptr(self):
        return self.tracked.data_ptr() + 24

    def ws(self, nbytes):
        buf, mask, off = G.workspace(nbytes)
        buf = buf.to(DEV)
        self.spaces.append((buf, mask.to(DEV)))
        return buf.data_ptr() + off

    def get(self, name):
        return self.a.view(name, self.bufs[name])

    def done(self, written, what):
        """After a call (or several): slack of what was written, everything else untouched."""
        torch.cuda.synchronize()
        for n, buf in self.bufs.items():
            if not self.a.is_out[n]:
                continue
            if n in written:
                G.check_slack(buf, self.pr.masks[n], f"{self.what} {what} {n}")
                assert not torch.isnan(self.get(n).float()).any().item(), f"{self.what} {what} {n}: an unwritten element"
            else:
                assert torch.equal(buf.view(torch.int32), self.pr.bufs0[n].view(torch.int32)), \
                    f"{self.what} {what}: {n} was not given to the call and changed"
        for buf, mask in self.spaces:
            G.check_slack(buf, mask, f"{self.what} {what} workspace guard")
        bad = self.tracked.clone()
        bad[3] = GUARD64
        assert (bad == GUARD64).all().item(), f"{self.what} {what}: words around num_batches_tracked written"

    def ref(self, name):
        dev = self.pr.dev
        if name not in dev:
            dev[name] = (self.p.ref[name].to(DEV), self.p.scale[name].to(DEV))
        return dev[name]

    def check(self, out, name, what, ref=None, scale=None):
        r, s = self.ref(name)
        G.check(name, self.get(out), r if ref is None else ref.to(DEV), s if scale is None else scale.to(DEV),
                f"{self.what} {what} [{out}]", report=True)

    def check16(self, out16, out, what):
        got, want = self.get(out16), self.get(out).to(torch.bfloat16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            f"{self.what} {what}: {out16} is not the RNE bf16 rounding of {out} " \
            f"({int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ)"


def call(L, rc, what):
    torch.cuda.synchronize()
    L.check(rc, what)


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
def ln_fwd16(x, y16="y16", mean="mean", rstd="rstd", rows=None, C=None, y16_extra=0):
    p = x.p
    return x.lib.mdemi_layernorm_fwd16(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr(y16, y16_extra),
                                       x.ptr(mean), x.ptr(rstd), rows or p.rows, C or p.C, p.eps, x.L.stream())


def ln_bwd(x, dx="dx", dgamma="dgamma", dbeta="dbeta", accumulate=0, rows=None, C=None, workspace=True):
    p = x.p
    ws = x.ws(x.lib.mdemi_layernorm_bwd_workspace_size(p.rows, p.C)) if workspace else None
    return x.lib.mdemi_layernorm_bwd(x.ptr("dy"), x.ptr("x"), x.ptr("mean_in"), x.ptr("rstd_in"), x.ptr("gamma"),
                                     x.ptr(dx), x.ptr(dgamma), x.ptr(dbeta), rows or p.rows, C or p.C, accumulate, ws,
                                     x.L.stream())


def ln_bwd_add(x, dadd, dx, rows=None, C=None):
    p = x.p
    ws = x.ws(x.lib.mdemi_layernorm_bwd_workspace_size(p.rows, p.C))
    return x.lib.mdemi_layernorm_bwd_add(x.ptr("dy"), x.ptr("x"), x.ptr("mean_in"), x.ptr("rstd_in"), x.ptr("gamma"),
                                         x.ptr(dadd), x.ptr(dx), x.ptr("dgamma"), x.ptr("dbeta"), rows or p.rows,
                                         C or p.C, ws, x.L.stream())


@pytest.mark.parametrize("case", G.LN_CASES + G.LN_EXACT_CASES, ids=lambda c: c.name)
def test_layernorm(L, case):
    """Every ln_cache instantiation with a partly filled and with a full last float4 group, 5 rows
    (idle waves in the last block), 1 and 3 rows, and the grid-stride shapes: the forward with
    y16 / mean / rstd, then the backward with dgamma and dbeta."""
    x = Run(L, case)
    call(L, ln_fwd16(x), "layernorm_fwd16")
    for n in ("y", "mean", "rstd"):
        x.check(n, "ln." + n, "forward")
    x.check16("y16", "y", "forward")
    x.done({"y", "y16", "mean", "rstd"}, "forward")
    if case.kind == "const":     # the mean is exact: y is beta bit for bit, rstd = 1 / sqrt(eps) to 1 ulp
        assert torch.equal(x.get("y"), x.p.beta.float().to(DEV)[None, :].expand(case.rows, case.C))
        assert torch.equal(x.get("mean"), torch.tensor(G.CONST_VALUES, device=DEV))
        want = torch.full((case.rows,), float(torch.tensor(x.p.eps, dtype=torch.float32).double().rsqrt()), device=DEV)
        got = x.get("rstd")
        assert ((got == want) | (got == torch.nextafter(want, want * 2)) | (got == torch.nextafter(want, want * 0))).all()
    if case.kind == "alt":       # mean 0 and variance 1 exactly: y is +-rstd bit for bit
        assert torch.equal(x.get("mean"), torch.zeros(case.rows, device=DEV))
        assert torch.equal(x.get("y"), x.p.x.float().to(DEV) * x.get("rstd")[:, None])
    if not case.backward:
        return
    call(L, ln_bwd(x), "layernorm_bwd")
    for n in ("dx", "dgamma", "dbeta"):
        x.check(n, "ln." + n, "backward")
    x.done({"y", "y16", "mean", "rstd", "dx", "dgamma", "dbeta"}, "backward")


def test_layernorm_forward_arms(L):
    """mean / rstd NULL; y16 given and NULL with the same fp32 y; mdemi_layernorm_fwd."""
    full = Run(L, G.LN_ARMS)
    call(L, ln_fwd16(full), "layernorm_fwd16")
    bare = Run(L, G.LN_ARMS)
    call(L, ln_fwd16(bare, y16=None, mean=None, rstd=None), "layernorm_fwd16 (y16, mean, rstd NULL)")
    bare.check("y", "ln.y", "mean / rstd NULL")
    bare.done({"y"}, "mean / rstd NULL")
    assert torch.equal(full.get("y"), bare.get("y"))
    for skip in ("mean", "rstd"):
        one = Run(L, G.LN_ARMS)
        keep = "rstd" if skip == "mean" else "mean"
        call(L, ln_fwd16(one, **{skip: None}), f"layernorm_fwd16 ({skip} NULL)")
        one.check(keep, "ln." + keep, f"{skip} NULL")
        one.check16("y16", "y", f"{skip} NULL")
        one.done({"y", "y16", keep}, f"{skip} NULL")
    plain, p = Run(L, G.LN_ARMS), full.p
    call(L, plain.lib.mdemi_layernorm_fwd(plain.ptr("x"), plain.ptr("gamma"), plain.ptr("beta"), plain.ptr("y"),
                                          plain.ptr("mean"), plain.ptr("rstd"), p.rows, p.C, p.eps, L.stream()),
         "layernorm_fwd")
    plain.done({"y", "mean", "rstd"}, "layernorm_fwd")
    for n in ("y", "mean", "rstd"):
        assert torch.equal(plain.get(n), full.get(n)), n


@pytest.mark.parametrize("dgamma,dbeta", [("dgamma", None), (None, "dbeta"), (None, None), ("dgamma", "dbeta")])
def test_layernorm_backward_parameter_arms(L, dgamma, dbeta):
    x = Run(L, G.LN_ARMS)
    call(L, ln_bwd(x, dgamma=dgamma, dbeta=dbeta), "layernorm_bwd")
    given = {n for n in ("dx", dgamma, dbeta) if n}
    for n in given:
        x.check(n, "ln." + n, f"dgamma {dgamma} dbeta {dbeta}")
    x.done(given, f"dgamma {dgamma} dbeta {dbeta}")


def test_layernorm_accumulate_and_add(L):
    """accumulate_dx = 1 adds into what dx holds; bwd_add adds dadd, also where dadd is dx."""
    p = G.ln_problem(G.LN_ARMS)
    ref, scale = p.ref["ln.dx"] + p.dx0, G.ln_dx_scale(p, p.dx0)
    x = Run(L, G.LN_ARMS)
    call(L, ln_bwd(x, dx="dx_acc", accumulate=1), "layernorm_bwd accumulate_dx")
    x.check("dx_acc", "ln.dx", "accumulate_dx = 1", ref, scale)
    x.done({"dx_acc", "dgamma", "dbeta"}, "accumulate_dx = 1")
    x = Run(L, G.LN_ARMS)
    call(L, ln_bwd(x, dx="dx_acc", accumulate=0), "layernorm_bwd")
    x.check("dx_acc", "ln.dx", "accumulate_dx = 0 over old contents")
    x = Run(L, G.LN_ARMS)
    call(L, ln_bwd_add(x, "dx_acc", "dx_acc"), "layernorm_bwd_add (dadd == dx)")
    x.check("dx_acc", "ln.dx", "bwd_add aliased", ref, scale)
    for n in ("dgamma", "dbeta"):
        x.check(n, "ln." + n, "bwd_add aliased")
    x.done({"dx_acc", "dgamma", "dbeta"}, "bwd_add aliased")
    x = Run(L, G.LN_ARMS)
    call(L, ln_bwd_add(x, "dadd", "dx"), "layernorm_bwd_add")
    x.check("dx", "ln.dx", "bwd_add", p.ref["ln.dx"] + p.dadd, G.ln_dx_scale(p, p.dadd))
    x.done({"dx", "dgamma", "dbeta"}, "bwd_add")


@pytest.mark.parametrize("why,C,code", [("C % 4 != 0", 6, EINVAL), ("C > 6144", 6148, EINVAL)])
def test_layernorm_rejects_unsupported_widths(L, why, C, code):
    """2 rows of C channels inside the 37 x 384 allocations: an error code, nothing written."""
    x = Run(L, G.LN_ARMS)
    assert 2 * C <= x.p.rows * x.p.C
    assert ln_fwd16(x, rows=2, C=C) == code
    assert ln_bwd(x, rows=2, C=C) == code
    assert ln_bwd_add(x, "dadd", "dx", rows=2, C=C) == code
    x.done(set(), why)


def test_layernorm_rejects_bad_pointers(L):
    x = Run(L, G.LN_ARMS)
    assert ln_bwd(x, workspace=False) == EWORKSPACE
    assert ln_bwd_add(x, None, "dx") == EINVAL
    assert ln_fwd16(x, y16_extra=2) == EINVAL          # y16 2-B aligned
    assert ln_fwd16(x, y16_extra=4) == EINVAL          # 4-B aligned
    x.done(set(), "bad pointers")
    assert x.lib.mdemi_last_error()


# ---------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------
def _bn_ws(x):
    p = x.p
    return x.ws(x.lib.mdemi_chnorm_workspace_size(p.N, p.HW, p.C, p.C, 1))


def bn_train(x, y16, tracked, pooled=False):
    p, lib = x.p, x.lib
    head = (x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr(y16))
    tail = (x.ptr("mean"), x.ptr("rstd"), x.ptr("running_mean"), x.ptr("running_var"),
            x.tracked_ptr() if tracked else None, p.momentum, p.N, p.HW, p.C, p.eps, p.act)
    if pooled:
        ws = x.ws(lib.mdemi_bn_train_fwd_pooled_workspace_size(p.N, p.HW, p.C))
        return lib.mdemi_bn_train_fwd_pooled(*head, x.ptr("pooled"), *tail, ws, x.L.stream())
    if y16 is None:
        return lib.mdemi_bn_train_fwd(*head[:4], *tail, _bn_ws(x), x.L.stream())
    return lib.mdemi_bn_train_fwd16(*head, *tail, _bn_ws(x), x.L.stream())


def _check_train(x, what, tracked, y16):
    for n in ("y", "mean", "rstd", "running_mean", "running_var"):
        x.check(n, "bn." + n, what)
    if y16:
        x.check16("y16", "y", what)
    assert x.tracked[3].item() == G.TRACKED0 + (1 if tracked else 0), f"{x.what} {what}: num_batches_tracked"


@pytest.mark.parametrize("case", G.BN_CASES, ids=lambda c: c.name)
def test_batchnorm_forward(L, case):
    """mdemi_chnorm_fwd; mdemi_bn_train_fwd16 with y16 and num_batches_tracked, mdemi_bn_train_fwd
    without either (the same fp32 y); mdemi_bn_train_fwd_pooled on the aligned C % 4 == 0 cases (y
    bit for bit that of bn_train_fwd16); mdemi_bn_running_update with and without the counter."""
    p = G.bn_problem(case)
    has16 = "y16" in prepared(case).a.bufs
    x = Run(L, case)
    call(L, x.lib.mdemi_chnorm_fwd(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr("mean"), x.ptr("rstd"),
                                   p.N, p.HW, p.C, p.C, 1, p.eps, p.act, _bn_ws(x), L.stream()), "chnorm_fwd")
    for n in ("y", "mean", "rstd"):
        x.check(n, "bn." + n, "chnorm_fwd")
    x.done({"y", "mean", "rstd"}, "chnorm_fwd")
    plain_y = x.get("y").clone()

    x = Run(L, case)
    call(L, bn_train(x, "y16" if has16 else None, True), "bn_train_fwd16")
    _check_train(x, "bn_train_fwd16", True, has16)
    x.done({"y", "mean", "rstd", "running_mean", "running_var"} | ({"y16"} if has16 else set()), "bn_train_fwd16")
    assert torch.equal(x.get("y"), plain_y)

    b = Run(L, case)
    call(L, bn_train(b, None, False), "bn_train_fwd")
    _check_train(b, "bn_train_fwd (no counter)", False, False)
    b.done({"y", "mean", "rstd", "running_mean", "running_var"}, "bn_train_fwd (no counter)")
    for n in ("y", "mean", "rstd", "running_mean", "running_var"):
        assert torch.equal(x.get(n), b.get(n)), n

    if case.pooled:
        b = Run(L, case)
        call(L, bn_train(b, "y16", True, pooled=True), "bn_train_fwd_pooled")
        _check_train(b, "bn_train_fwd_pooled", True, True)
        b.check("pooled", "bn.pooled", "bn_train_fwd_pooled")
        b.done({"y", "y16", "pooled", "mean", "rstd", "running_mean", "running_var"}, "bn_train_fwd_pooled")
        for n in ("y", "mean", "rstd", "running_mean", "running_var"):
            assert torch.equal(x.get(n), b.get(n)), f"{n}: bn_train_fwd_pooled and bn_train_fwd16 differ"

    for tracked in (True, False):
        u = Run(L, case)
        call(L, u.lib.mdemi_bn_running_update(u.ptr("mean_in"), u.ptr("rstd_in"), u.ptr("running_mean"),
                                              u.ptr("running_var"), u.tracked_ptr() if tracked else None, p.C, p.rows,
                                              p.eps, p.momentum, L.stream()), "bn_running_update")
        u.check("running_mean", "bn.ru_running_mean", "bn_running_update")
        u.check("running_var", "bn.ru_running_var", "bn_running_update")
        assert u.tracked[3].item() == G.TRACKED0 + (1 if tracked else 0)
        u.done({"running_mean", "running_var"}, "bn_running_update")


@pytest.mark.parametrize("case", G.BN_CASES, ids=lambda c: c.name)
def test_batchnorm_backward(L, case):
    """mdemi_chnorm_bwd16 with dx16 and without (the same fp32 dx); mdemi_bn_frozen_bwd with dx
    NULL and with dgamma / dbeta (and the workspace) NULL."""
    p = G.bn_problem(case)
    has16 = "dx16" in prepared(case).a.bufs

    def bwd(x, dx16):
        return x.lib.mdemi_chnorm_bwd16(x.ptr("dy"), x.ptr("x"), x.ptr("y"), x.ptr("mean_in"), x.ptr("rstd_in"),
                                        x.ptr("gamma"), x.ptr("beta"), x.ptr("dx"), x.ptr(dx16), x.ptr("dgamma"),
                                        x.ptr("dbeta"), p.N, p.HW, p.C, p.C, 1, p.act, _bn_ws(x), L.stream())

    x = Run(L, case)
    call(L, bwd(x, "dx16" if has16 else None), "chnorm_bwd16")
    for n in ("dx", "dgamma", "dbeta"):
        x.check(n, "bn." + n, "chnorm_bwd16")
    if has16:
        x.check16("dx16", "dx", "chnorm_bwd16")
    x.done({"dx", "dgamma", "dbeta"} | ({"dx16"} if has16 else set()), "chnorm_bwd16")
    b = Run(L, case)
    call(L, bwd(b, None), "chnorm_bwd16 (dx16 NULL)")
    b.done({"dx", "dgamma", "dbeta"}, "chnorm_bwd16 (dx16 NULL)")
    for n in ("dx", "dgamma", "dbeta"):
        assert torch.equal(x.get(n), b.get(n)), n

    def frozen(x, dx, dgamma, dbeta, ws):
        return x.lib.mdemi_bn_frozen_bwd(x.ptr("dy"), x.ptr("x"), x.ptr("mean_in"), x.ptr("rstd_in"), x.ptr("gamma"),
                                         x.ptr("beta"), x.ptr(dx), x.ptr(dgamma), x.ptr(dbeta), p.N, p.HW, p.C, p.act,
                                         _bn_ws(x) if ws else None, L.stream())

    f = Run(L, case)
    call(L, frozen(f, None, "dgamma", "dbeta", True), "bn_frozen_bwd (dx NULL)")
    for n in ("dgamma", "dbeta"):
        f.check(n, "bn." + n, "bn_frozen_bwd (dx NULL)")
    f.done({"dgamma", "dbeta"}, "bn_frozen_bwd (dx NULL)")
    f = Run(L, case)
    call(L, frozen(f, "dx", None, None, False), "bn_frozen_bwd (dgamma / dbeta NULL)")
    f.check("dx", "bn.frozen_dx", "bn_frozen_bwd (dgamma / dbeta NULL)")
    f.done({"dx"}, "bn_frozen_bwd (dgamma / dbeta NULL)")
    f = Run(L, case)
    assert frozen(f, "dx", "dgamma", None, True) == EINVAL
    assert frozen(f, "dx", "dgamma", "dbeta", False) == EWORKSPACE
    f.done(set(), "bn_frozen_bwd refused")


def test_misaligned_case_is_misaligned(L):
    """x / y / dy / dx of the fallback case sit 4 B off a 16-B boundary on the device, the bf16
    copies 8 B off one, everything else on one."""
    x = Run(L, G.BN_MISALIGNED)
    for n in ("x", "y", "dy", "dx"):
        assert x.ptr(n) % 16 == 4, n
    for n in ("y16", "dx16"):
        assert x.ptr(n) % 16 == 8, n
    for n in ("gamma", "beta", "mean", "rstd", "mean_in", "rstd_in", "dgamma", "dbeta", "running_mean", "running_var"):
        assert x.ptr(n) % 16 == 0, n
    a = Run(L, G.BN_VECTOR_CASES[0])
    assert all(a.ptr(n) % 16 == 0 for n in ("x", "y", "dy", "dx")) and a.ptr("y16") % 16 == 8


# ---------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.GN_CASES, ids=lambda c: c.name)
def test_groupnorm(L, case):
    """Forward, backward and mdemi_chnorm_apply: groups of 2, 8, 15, 72 and 180 elements (fewer than
    the block's 256 threads) and of 4,800 (more), one channel per group, one group per sample."""
    p = G.gn_problem(case)
    x = Run(L, case)
    ws = x.ws(x.lib.mdemi_chnorm_workspace_size(p.N, p.HW, p.C, p.groups, 0))
    call(L, x.lib.mdemi_chnorm_fwd(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr("mean"), x.ptr("rstd"),
                                   p.N, p.HW, p.C, p.groups, 0, p.eps, p.act, ws, L.stream()), "chnorm_fwd")
    for n in ("y", "mean", "rstd"):
        x.check(n, "gn." + n, "chnorm_fwd")
    x.done({"y", "mean", "rstd"}, "chnorm_fwd")
    ws = x.ws(x.lib.mdemi_chnorm_workspace_size(p.N, p.HW, p.C, p.groups, 0))
    call(L, x.lib.mdemi_chnorm_bwd(x.ptr("dy"), x.ptr("x"), x.ptr("y"), x.ptr("mean_in"), x.ptr("rstd_in"),
                                   x.ptr("gamma"), x.ptr("beta"), x.ptr("dx"), x.ptr("dgamma"), x.ptr("dbeta"), p.N, p.HW,
                                   p.C, p.groups, 0, p.act, ws, L.stream()), "chnorm_bwd")
    for n in ("dx", "dgamma", "dbeta"):
        x.check(n, "gn." + n, "chnorm_bwd")
    x.done({"y", "mean", "rstd", "dx", "dgamma", "dbeta"}, "chnorm_bwd")
    a = Run(L, case)
    call(L, a.lib.mdemi_chnorm_apply(a.ptr("x"), a.ptr("gamma"), a.ptr("beta"), a.ptr("mean_in"), a.ptr("rstd_in"),
                                     a.ptr("y"), p.N, p.HW, p.C, p.groups, 0, p.act, L.stream()), "chnorm_apply")
    a.check("y", "gn.apply_y", "chnorm_apply")
    a.done({"y"}, "chnorm_apply")


def test_channel_norm_refusals(L):
    """Outside the contract: the header's code and nothing written.  mdemi_bn_train_fwd_pooled on
    C % 4 != 0 and on misaligned x / y; a 4-B aligned y16 / dx16; BatchNorm without a workspace;
    GroupNorm with C % groups != 0."""
    for case in (G.BN_SCALAR_CASES[0], G.BN_MISALIGNED):
        x = Run(L, case)
        assert bn_train(x, "y16", True, pooled=True) == EINVAL
        x.done(set(), "bn_train_fwd_pooled refused")
    x, p = Run(L, G.BN_VECTOR_CASES[0]), G.bn_problem(G.BN_VECTOR_CASES[0])
    stats = (x.ptr("mean"), x.ptr("rstd"), x.ptr("running_mean"), x.ptr("running_var"), x.tracked_ptr(), p.momentum,
             p.N, p.HW, p.C, p.eps, p.act)
    assert x.lib.mdemi_bn_train_fwd16(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr("y16", 4), *stats,
                                      _bn_ws(x), L.stream()) == EINVAL
    assert x.lib.mdemi_bn_train_fwd(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), *stats, None,
                                    L.stream()) == EWORKSPACE
    assert x.lib.mdemi_chnorm_bwd16(x.ptr("dy"), x.ptr("x"), x.ptr("y"), x.ptr("mean_in"), x.ptr("rstd_in"),
                                    x.ptr("gamma"), x.ptr("beta"), x.ptr("dx"), x.ptr("dx16", 4), x.ptr("dgamma"),
                                    x.ptr("dbeta"), p.N, p.HW, p.C, p.C, 1, p.act, _bn_ws(x), L.stream()) == EINVAL
    x.done(set(), "BatchNorm refused")
    assert x.tracked[3].item() == G.TRACKED0
    case = G.GN_CASES[-1]
    x, p = Run(L, case), G.gn_problem(case)
    ws = x.ws(x.lib.mdemi_chnorm_workspace_size(p.N, p.HW, p.C, 5, 0))
    assert p.C % 5 != 0
    assert x.lib.mdemi_chnorm_fwd(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("y"), x.ptr("mean"), x.ptr("rstd"),
                                  p.N, p.HW, p.C, 5, 0, p.eps, p.act, ws, L.stream()) == EINVAL
    assert x.lib.mdemi_chnorm_bwd(x.ptr("dy"), x.ptr("x"), x.ptr("y"), x.ptr("mean_in"), x.ptr("rstd_in"), x.ptr("gamma"),
                                  x.ptr("beta"), x.ptr("dx"), x.ptr("dgamma"), x.ptr("dbeta"), p.N, p.HW, p.C, 5, 0,
                                  p.act, ws, L.stream()) == EINVAL
    assert x.lib.mdemi_chnorm_apply(x.ptr("x"), x.ptr("gamma"), x.ptr("beta"), x.ptr("mean_in"), x.ptr("rstd_in"),
                                    x.ptr("y"), p.N, p.HW, p.C, 5, 0, p.act, L.stream()) == EINVAL
    x.done(set(), "GroupNorm refused")
