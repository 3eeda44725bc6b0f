"""The window-attention descriptor contract (mdemi_winattn_desc, include/mdemi.h) against the
fp64 reference of tests/winattn_contract_ref.py, through the C ABI itself (ctypes), so leading
dimensions, null pointers and entry points vary on their own.

Every launch works on views into larger allocations the test owns (winattn_contract_cases.build):
NaN around the inputs, a quiet-NaN pattern in the outputs and around them.  After the call
  * every output meets the per-block criterion of winattn_contract_cases.check (tolerances: 4 x
    the error of the reference's own fp32 restatement, not measured on the kernel);
  * no owned element is NaN: d_rpb_table and every given pad sum were written in full;
  * every slack word -- rows past B*H*W, columns past heads * 32 -- still holds the pattern.
The exact-gather cases pin index maps, head slices, bias orientation and the pad-vector path
bit for bit."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import winattn_contract_cases as G
import winattn_contract_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope="module")
def L():
    from mdemi import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=8)
def prepared(case):
    """The case's allocations on the device (outputs pristine: cloned per launch) and its
    reference, computed once on the CPU in fp64."""
    d = G.build(case)
    return SimpleNamespace(case=case, d=d, ref=G.problem(case).ref, inputs={n: t.to(DEV) for n, t in d.inputs.items()},
                           outputs0={n: t.to(DEV) for n, t in d.outputs.items()},
                           masks={n: m.to(DEV) for n, m in d.masks.items()})


class Launch:
    """One forward (+ backward) of a case on fresh output allocations."""

    def __init__(self, L, case, drop=(), **overrides):
        self.L, self.lib, self.pr, self.case = L, L.load(), prepared(case), case
        self.outs = {n: t.clone() for n, t in self.pr.outputs0.items()}
        self.drop, self.overrides = set(drop), overrides
        self.fwd_ws = self.bwd_ws = None

    def desc(self, backward):
        c, dd, d = self.case, self.pr.d, self.L.WinAttnDesc()

        def at(name):
            if name in self.drop or name not in dd.at:
                return None
            alloc, off = dd.at[name]
            buf = self.outs[alloc] if alloc in self.outs else self.pr.inputs[alloc]
            return buf.data_ptr() + 4 * off

        d.B, d.H, d.W, d.heads, d.head_dim, d.window, d.shift, d.scale = c.B, c.H, c.W, c.heads, R.HD, R.WS, c.shift, c.scale
        d.q, d.k, d.qk_ld, d.q_pad, d.k_pad = at("q"), at("k"), dd.qk_ld, at("q_pad"), at("k_pad")
        d.v, d.v_ld, d.v_pad, d.rpb_table = at("v"), dd.v_ld, at("v_pad"), at("rpb_table")
        d.out, d.out_ld, d.lse, d.sample_live = at("out"), dd.out_ld, at("lse"), at("sample_live")
        if backward:
            d.dout, d.dq, d.dk, d.dqk_ld, d.dv, d.dv_ld = at("dout"), at("dq"), at("dk"), dd.dqk_ld, at("dv"), dd.dv_ld
            d.d_rpb_table, d.dq_pad, d.dk_pad, d.dv_pad = at("d_rpb_table"), at("dq_pad"), at("dk_pad"), at("dv_pad")
        for k, v in self.overrides.items():
            setattr(d, k, v)
        return d

    @staticmethod
    def _ws(nbytes):  # NaN-filled: a workspace word read before it is written shows
        return torch.full((max(nbytes, 4) + 3 >> 2,), float("nan"), device=DEV)

    def forward(self, short=0):
        d = self.desc(False)
        need = self.lib.mdemi_winattn_fwd_workspace_size(ctypes.byref(d))
        self.fwd_ws = self._ws(need)
        d.workspace, d.workspace_bytes = self.fwd_ws.data_ptr(), need - short
        rc = self.lib.mdemi_winattn_fwd(ctypes.byref(d), self.L.stream())
        torch.cuda.synchronize()
        return rc

    def backward(self, entry="bias_fwd", short=0):
        d = self.desc(True)
        need = self.lib.mdemi_winattn_bwd_workspace_size(ctypes.byref(d))
        self.bwd_ws = self._ws(need)
        d.workspace, d.workspace_bytes = self.bwd_ws.data_ptr(), need - short
        if entry == "plain":
            rc = self.lib.mdemi_winattn_bwd(ctypes.byref(d), self.L.stream())
        else:
            bias = self.fwd_ws.data_ptr() if entry == "bias_fwd" else None
            rc = self.lib.mdemi_winattn_bwd_bias(ctypes.byref(d), bias, self.L.stream())
        torch.cuda.synchronize()
        return rc

    # ---- reading the outputs back ----
    def get(self, name):
        d = self.pr.d
        if name in G.ROW_OUTPUTS:
            return G.owned(d, name, self.outs[d.cols[name][0]])
        n = self.pr.ref[name].numel()
        return self.outs[name][G.VOFF:G.VOFF + n]

    def untouched(self, names, what):
        for n in names:
            G.check_slack(self.outs[n], torch.zeros_like(self.pr.masks[n]), f"{what} {n} (must be untouched)")

    def slack(self, what):
        for n, buf in self.outs.items():
            G.check_slack(buf, self.pr.masks[n], f"{what} {n}")

    def given(self, names):
        return [n for n in names if n in G.ROW_OUTPUTS or n in self.outs]

    def check(self, names, what, select=None):
        for n in self.given(names):
            G.check(n, self.get(n), self.pr.ref, what, select=select)


def run(L, case, what=None, entry="bias_fwd"):
    """Forward and backward of `case`, every requirement of the module text asserted."""
    what = what or case.name
    x = Launch(L, case)
    L.check(x.forward(), "winattn_fwd")
    x.check(("out", "lse"), what + " forward")
    x.untouched([n for n in x.outs if n not in ("out", "lse")], what + " forward")
    x.slack(what + " forward")
    L.check(x.backward(entry), "winattn_bwd")
    x.check(G.BWD_OUTPUTS + ("out", "lse"), what)
    x.slack(what)
    return x


@pytest.mark.parametrize("case", G.geometry_cases(), ids=lambda c: c.name)
def test_geometry_occupancy(L, case):
    """Every geometry and shift, with nwin * heads % 4 in {0, 1, 2, 3}: full and partial last
    workgroups, down to a single (window, head) item on a single token.  The MIXED launch holds
    windows with and without pad tokens -- the backward's fast and slow path -- and is checked
    window by window."""
    x = run(L, case)
    if case.name != G.MIXED:
        return
    geom = x.pr.ref["geom"]
    kinds = set()
    for w in range(geom.nwin):
        rows = geom.row[w][geom.row[w] >= 0]
        kind = "fast" if rows.numel() == R.N else "slow"
        kinds.add(kind)
        x.check(G.ROW_OUTPUTS, f"{case.name} window {w} ({kind} path)", select=rows)
        G.check("lse", x.get("lse"), x.pr.ref, f"{case.name} window {w} ({kind} path)", select=torch.tensor([w]))
    assert kinds == {"fast", "slow"}


@pytest.mark.parametrize("case", G.layout_cases(), ids=lambda c: c.name)
def test_operand_layouts(L, case):
    """Swin-shared and CRF operands, a separate v with its pad vector, each pad vector null on its
    own and all null, leading dimensions wider than the data (q/k/v, out and dout, dq/dk, dv) and
    different between operand and gradient, each pad-sum output null and all null."""
    x = run(L, case)
    missing = [n for n in ("dq_pad", "dk_pad", "dv_pad") if not getattr(case, n)]
    assert all(n not in x.outs for n in missing)


@pytest.mark.parametrize("geo", list(G.LAYOUT_GEOMETRIES))
def test_forward_without_lse(L, geo):
    """lse == NULL on a forward-only call: out is bit-equal to the call that saves lse."""
    case = next(c for c in G.layout_cases() if c.name == f"{geo}-swin")
    a, b = Launch(L, case), Launch(L, case, drop=("lse",))
    L.check(a.forward(), "winattn_fwd")
    L.check(b.forward(), "winattn_fwd (lse NULL)")
    assert torch.equal(a.get("out"), b.get("out"))
    b.check(("out",), case.name + " lse NULL")
    b.untouched(["lse"], case.name + " lse NULL")
    b.slack(case.name + " lse NULL")


@pytest.mark.parametrize("case", G.gather_cases(), ids=lambda c: c.name)
def test_exact_gather(L, case):
    """q = k = 0 and a table of zeros but +80 at one relative offset: a query whose reference
    attention row is one-hot (max p >= 1 - 1e-30) must return the v row or pad vector the
    reference gathers, bit for bit; the other queries meet the criterion."""
    exact, want, _ = G.gather_expected(case)
    x = Launch(L, case)
    L.check(x.forward(), "winattn_fwd")
    got = x.get("out").cpu()
    if not torch.equal(got[exact], want[exact]):
        bad = (got != want).any(1) & exact
        r = bad.nonzero()[0].item()
        c = (got[r] != want[r]).nonzero()[0].item()
        raise AssertionError(f"{case.name}: {int(bad.sum())} of {int(exact.sum())} one-hot queries do not return the "
                             f"gathered row; first row {r} column {c}: got {got[r, c].item()!r}, want {want[r, c].item()!r}")
    x.check(("out", "lse"), case.name)
    x.slack(case.name)


ENTRY_CASE = "10x12s3-B1h5"   # 20 items, pad tokens and mask: LDS float atomics feed the pad sums


def _bits(x):
    return {n: t.view(torch.int32).clone() for n, t in x.outs.items()}


def test_entry_points_agree(L):
    """mdemi_winattn_bwd (expands the table again), mdemi_winattn_bwd_bias(NULL) and
    mdemi_winattn_bwd_bias(the forward's workspace) write the same bits everywhere."""
    case = next(c for c in G.geometry_cases() if c.name == ENTRY_CASE)
    results = {entry: _bits(run(L, case, f"{case.name} [{entry}]", entry)) for entry in ("plain", "bias_null", "bias_fwd")}
    for entry in ("bias_null", "bias_fwd"):
        for n, t in results["plain"].items():
            assert torch.equal(t, results[entry][n]), f"{n}: mdemi_winattn_bwd and {entry} differ"


@pytest.mark.parametrize("name", [ENTRY_CASE, G.MIXED, "3x20s1-B1h5"])
def test_backward_repeats_bit_for_bit(L, name):
    case = next(c for c in G.geometry_cases() if c.name == name)
    x = Launch(L, case)
    L.check(x.forward(), "winattn_fwd")
    L.check(x.backward(), "winattn_bwd")
    first = _bits(x)
    L.check(x.backward(), "winattn_bwd")
    for n, t in _bits(x).items():
        assert torch.equal(t, first[n]), f"{n}: a second launch of the same backward differs"


def test_workspace_one_byte_short(L):
    case = next(c for c in G.geometry_cases() if c.name == ENTRY_CASE)
    x = Launch(L, case)
    assert x.forward(short=1) == EWORKSPACE
    x.untouched(list(x.outs), "forward, workspace one byte short")
    L.check(x.forward(), "winattn_fwd")
    before = _bits(x)
    assert x.backward(short=1) == EWORKSPACE
    for n, t in _bits(x).items():
        assert torch.equal(t, before[n]), f"{n}: written by a backward that returned MDEMI_EWORKSPACE"


@pytest.mark.parametrize("why,fields", [("window 8", dict(window=8)), ("head_dim 16", dict(head_dim=16)),
                                        ("shift 7", dict(shift=7)), ("qk_ld % 4 != 0", dict(qk_ld=-1))])
def test_rejected_descriptors(L, why, fields):
    """Outside the contract: an error code from both entry points and nothing launched."""
    case = next(c for c in G.geometry_cases() if c.name == ENTRY_CASE)
    good = Launch(L, case)
    L.check(good.forward(), "winattn_fwd")
    if "qk_ld" in fields:
        fields = dict(qk_ld=good.pr.d.qk_ld + 2)
    x = Launch(L, case, **fields)
    d = x.desc(False)
    assert x.lib.mdemi_winattn_fwd_workspace_size(ctypes.byref(d)) == 0
    # workspaces of the valid descriptor's size: the refusal is not for want of one
    ws = Launch._ws(good.lib.mdemi_winattn_bwd_workspace_size(ctypes.byref(good.desc(True))))
    d.workspace, d.workspace_bytes = ws.data_ptr(), 4 * ws.numel()
    assert x.lib.mdemi_winattn_fwd(ctypes.byref(d), L.stream()) == EINVAL
    torch.cuda.synchronize()
    x.untouched(list(x.outs), why + " forward")
    x.outs["out"].copy_(good.outs["out"])
    x.outs["lse"].copy_(good.outs["lse"])
    before = _bits(x)
    d = x.desc(True)
    d.workspace, d.workspace_bytes = ws.data_ptr(), 4 * ws.numel()
    assert x.lib.mdemi_winattn_bwd(ctypes.byref(d), L.stream()) == EINVAL
    assert x.lib.mdemi_winattn_bwd_bias(ctypes.byref(d), None, L.stream()) == EINVAL
    torch.cuda.synchronize()
    for n, t in _bits(x).items():
        assert torch.equal(t, before[n]), f"{why}: {n} written by a refused call"


def test_dead_sample_in_a_partial_workgroup(L):
    """sample_live = [0, 1, 1] with B = 3, heads = 3 on 7x7 tokens: 9 items, so the last workgroup
    has one active wave, and sample 0 -- the sample that item 0 belongs to -- is dead.  Its q / k
    / v / dout rows are NaN, and its out rows are made NaN before the backward: the live samples
    meet the reference, the dead rows are zero, d_rpb_table and the pad sums hold no NaN."""
    case = G.DEAD
    assert G.nitems(case) % 4 == 1 and case.live[0] == 0.0
    x = Launch(L, case)
    L.check(x.forward(), "winattn_fwd")
    x.check(("out", "lse"), case.name + " forward")
    dead = G.problem(case).dead_rows.to(DEV)
    assert torch.equal(x.get("out")[dead], torch.zeros_like(x.get("out")[dead]))
    x.get("out")[dead] = float("nan")
    L.check(x.backward(), "winattn_bwd")
    x.check(G.BWD_OUTPUTS, case.name)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(x.get(n)[dead], torch.zeros_like(x.get(n)[dead])), n
    x.slack(case.name)
