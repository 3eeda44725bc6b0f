"""Cases, guard-banded buffers and the comparison criterion of the window-attention descriptor
contract tests (tests/test_winattn_contract_ref.py on the CPU, tests/test_winattn_contract_gpu.py
on the GPU).  Plain torch on the CPU; nothing of the library is imported.

problem(case) draws the logical data of a case and computes its fp64 reference once
(winattn_contract_ref.attention).  build(case) lays that data out as the case's descriptor says,
every tensor inside a larger allocation of its own (gemm_contract_cases._place): NaN in the
slack of the inputs, PATTERN -- a quiet NaN -- in the outputs and their slack.

Data: q, k, v, dout uniform in [-1, 1], the table and the pad vectors too; the last sample's and
the last head's v and dout are scaled by 1e-2, so block magnitudes differ by 100 within a tensor
and a whole-tensor max-norm would hide an error in the small blocks.

Criterion (check): an element passes when |got - ref64| <= tol * scale + TINY, judged per block.
  out, dv                    block = one token row of one head, scale = max |ref64| of the block
  dq, dk                     the same block, scale = its max of the fp64 sum of the absolute values
                             of the terms added into an element: scale * sum P (|V||dO| + |dO||O|) |K|
                             resp. |Q|.  The block's own max |ref64| does not do: the score
                             gradient P (dP - D) of a query that can attend one key only (the lone
                             token of a shift region, as in 3x20 shift 1) is zero by cancellation of
                             two rounded sums, so its true dq row is 1e-43 while any fp32 evaluation
                             of D = rowsum(dO o O) leaves 1e-8
  lse                        block = one element, scale = |ref64|
  d_rpb_table, dk/dv_pad     block = one element, scale = the fp64 sum of the absolute values of
                             the terms added into it (score gradients of the slot over every
                             window; the k / v gradient rows of the pad tokens)
  dq_pad                     exactly zero
TOL is 4 x the largest such normalised error of the fp32 restatement of the reference
(attention(dtype=float32) on the CPU) against the fp64 one over every case of this module,
rounded up to two digits; the factor stands for the kernel's different summation order and its
__expf / __logf / reciprocal.  MEASURED_FP32 records those maxima; the CPU test measures them
again and holds TOL to within a factor 2 of 4 x the fresh figure (an fp32 sum depends on the
BLAS and thread count of the machine) and to <= 1e-4, what test_window_attention grants.
Nothing here was measured on the kernel."""
import functools
from collections import Counter
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch

import winattn_contract_ref as R
from gemm_contract_cases import PATTERN, _place, _vector, check_slack, slack_damage  # noqa: F401

TINY = 1e-30
SMALL = 1e-2                # factor on the last sample's / the last head's v and dout

# fp32 restatement against fp64, max over all_cases() (test_winattn_contract_ref.py prints them)
MEASURED_FP32 = dict(out=7.712e-07, lse=4.078e-07, dq=1.302e-07, dk=1.497e-07, dv=6.518e-07, d_rpb_table=8.043e-06,
                     dk_pad=4.356e-06, dv_pad=8.072e-07)
TOL = dict(out=3.1e-06, lse=1.7e-06, dq=5.3e-07, dk=6.0e-07, dv=2.7e-06, d_rpb_table=3.3e-05, dk_pad=1.8e-05,
           dv_pad=3.3e-06, dq_pad=0.0)

ROW_OUTPUTS = ("out", "dq", "dk", "dv")
BWD_OUTPUTS = ("dq", "dk", "dv", "d_rpb_table", "dq_pad", "dk_pad", "dv_pad")


@dataclass(frozen=True)
class Case:
    name: str
    H: int
    W: int
    shift: int
    B: int
    heads: int
    shared_v: bool = True       # Swin: q | k | v are column slices of one buffer; else v has its own
    q_pad: bool = True
    k_pad: bool = True
    v_pad: bool = True
    qk_extra: int = 0           # columns of the q/k(/v) buffer beyond the data
    v_extra: int = 0            # columns of a separate v buffer beyond the data
    out_extra: int = 0          # out_ld - C (dout is laid out at out_ld too)
    dqk_extra: int = -1         # columns of the dq/dk(/dv) buffer beyond the data; -1: as qk_extra
    dv_extra: int = -1          # of a separate dv buffer; -1: as v_extra
    dq_pad: bool = True         # which pad-sum outputs are given
    dk_pad: bool = True
    dv_pad: bool = True
    gather: tuple = None        # exact gather: (dy, dx) of the one table slot holding +80
    live: tuple = None          # sample_live
    seed: int = 0

    @property
    def C(self):
        return self.heads * R.HD

    @property
    def rows(self):
        return self.B * self.H * self.W

    @property
    def scale(self):
        return R.HD ** -0.5

    def data_key(self):
        """What the logical data and the reference depend on (layouts share them)."""
        return (self.H, self.W, self.shift, self.B, self.heads, self.q_pad, self.k_pad, self.v_pad, self.gather,
                self.live, self.seed)


def _uniform(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _dense(t):
    return R.Operand(t.reshape(-1), t.shape[1], 0)


@functools.lru_cache(maxsize=None)
def _problem(key):
    H, W, shift, B, heads, has_q, has_k, has_v, gather, live, seed = key
    C, rows = heads * R.HD, B * H * W
    g = torch.Generator().manual_seed(7000 + seed)
    p = SimpleNamespace(B=B, H=H, W=W, shift=shift, heads=heads, C=C, rows=rows, scale=R.HD ** -0.5)
    if gather is None:
        p.q, p.k, p.v = _uniform(g, rows, C), _uniform(g, rows, C), _uniform(g, rows, C)
        p.rpb = _uniform(g, R.T, heads)
        pads = [_uniform(g, C) for _ in range(3)]
    else:
        p.q, p.k = torch.zeros(rows, C, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64)
        p.v = torch.randint(1, 9, (rows, C), generator=g).double()
        p.rpb = torch.zeros(R.T, heads, dtype=torch.float64)
        p.rpb[(gather[0] + R.WS - 1) * (2 * R.WS - 1) + gather[1] + R.WS - 1] = 80.0
        pads = [_uniform(g, C), _uniform(g, C), torch.randint(1, 9, (C,), generator=g).double()]
    p.q_pad, p.k_pad, p.v_pad = [x if has else None for x, has in zip(pads, (has_q, has_k, has_v))]
    p.dout = _uniform(g, rows, C)
    if gather is None:
        small = torch.ones(B, 1, heads, 1, dtype=torch.float64)
        if B > 1:
            small[-1] = SMALL
        if heads > 1:
            small[:, :, -1] = SMALL
        for name in ("v", "dout"):
            t = getattr(p, name)
            setattr(p, name, (t.view(B, H * W, heads, R.HD) * small).reshape(rows, C))
    # what the kernels read is fp32: the reference works on the same numbers
    for name in ("q", "k", "v", "rpb", "q_pad", "k_pad", "v_pad", "dout"):
        if getattr(p, name) is not None:
            setattr(p, name, getattr(p, name).float().double())
    if live is not None:  # the reference of a masked call: a dead sample's dout is zero, its out rows are zero
        dead = (torch.tensor(live) == 0).repeat_interleave(H * W)
        p.dout_ref = torch.where(dead[:, None], torch.zeros_like(p.dout), p.dout)
    else:
        dead, p.dout_ref = None, p.dout
    p.dead_rows = dead
    p.ref = reference(p, torch.float64)
    return p


def problem(case):
    return _problem(case.data_key())


def reference(p, dtype, flaws=()):
    """out, lse and every backward output of problem p in `dtype` (float64: the reference;
    float32: its restatement, for TOL and the discrimination test)."""
    r = R.attention(_dense(p.q), _dense(p.k), _dense(p.v), p.q_pad, p.k_pad, p.v_pad, p.rpb, p.B, p.H, p.W, p.heads,
                    R.WS, p.shift, p.scale, dtype=dtype, flaws=flaws)
    res = dict(out=r.out, lse=r.lse, P=r.P, geom=r.geom)
    res.update(r.backward(p.dout_ref))
    if p.dead_rows is not None:
        res["out"] = torch.where(p.dead_rows[:, None], torch.zeros_like(res["out"]), res["out"])
        dead_win = p.dead_rows.view(p.B, -1)[:, 0].repeat_interleave(r.geom.nwin_per_sample)
        res["lse"] = torch.where(dead_win[:, None, None], torch.zeros_like(res["lse"]), res["lse"])
    return res


# ---------------------------------------------------------------------------------------------
# Criterion
# ---------------------------------------------------------------------------------------------
def block_scale(name, ref):
    """float64 scale of every element of output `name` (ref: the fp64 reference dict)."""
    want = ref[name]
    if name in ROW_OUTPUTS:
        rows, C = want.shape
        mag = ref[name + "_scale"] if name in ("dq", "dk") else want.abs()
        return mag.view(rows, C // R.HD, R.HD).amax(-1, keepdim=True).expand(-1, -1, R.HD).reshape(rows, C)
    if name == "lse":
        return torch.where(torch.isinf(want), torch.zeros_like(want), want.abs())
    if name == "dq_pad":
        return torch.zeros_like(want)
    return ref[name + "_scale"]


def normalised_error(name, got, ref):
    """max over elements of (|got - ref| - TINY) / scale, the smallest tol that passes check()
    (inf if an element of scale 0 differs by more than TINY)."""
    want, scale = ref[name], block_scale(name, ref)
    got = got.double().reshape(want.shape)
    same_inf = torch.isinf(want) & (got == want)
    err = torch.where(same_inf, torch.zeros_like(want), (got - want).abs())
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    zero = scale == 0
    if (err[zero] > TINY).any().item():
        return float("inf")
    return ((err[~zero] - TINY).clamp(min=0) / scale[~zero]).max().item() if (~zero).any().item() else 0.0


def check(name, got, ref, what, tol=None, select=None):
    """Assert the criterion for output `name`; `select` (a bool mask or index over the first
    dimension) restricts it to some rows.  got may live on any device."""
    tol = TOL[name] if tol is None else tol
    want, scale = ref[name], block_scale(name, ref)
    got = got.detach().double().cpu().reshape(want.shape)
    if select is not None:
        got, want, scale = got[select], want[select], scale[select]
    assert not torch.isnan(got).any().item(), f"{what} {name}: NaN in an owned element (unwritten, or slack was read)"
    same_inf = torch.isinf(want) & (got == want)
    err = torch.where(same_inf, torch.zeros_like(want), (got - want).abs())
    bound = tol * scale + TINY
    if not (err <= bound).all().item():
        bad = (~(err <= bound)).nonzero()
        i = tuple(bad[0].tolist())
        worst = (err / bound)[~(err <= bound)].max().item()
        raise AssertionError(f"{what} {name}: {bad.shape[0]} of {got.numel()} elements out of tolerance (tol {tol:.2e}"
                             f" per block, worst {worst:.3g} x the bound); first at {i}: got {got[i].item()!r}, want "
                             f"{want[i].item()!r}, |err| {err[i].item():.3e} > {bound[i].item():.3e}")


def passes(name, got, ref, tol=None):
    try:
        check(name, got, ref, "", tol)
        return True
    except AssertionError:
        return False


# ---------------------------------------------------------------------------------------------
# Buffers
# ---------------------------------------------------------------------------------------------
OFF = 8       # element offset of every matrix in its allocation (16-B aligned)
VOFF = 4      # of every vector


def build(case):
    """The CPU allocations of `case`: d.inputs / d.outputs name -> allocation, d.masks name ->
    owned elements of an output allocation, d.at name -> (allocation name, element offset) of each
    descriptor pointer, and the leading dimensions.  Outputs hold PATTERN everywhere."""
    c, p = case, problem(case)
    C, rows = c.C, c.rows
    d = SimpleNamespace(case=c, inputs={}, outputs={}, masks={}, at={})

    def matrix(name, cols_data, extra, values=None):
        ld = cols_data + extra
        output = values is None
        vals = torch.zeros(1, rows, cols_data, dtype=torch.float64) if output else values.reshape(1, rows, cols_data)
        buf, mask = _place(vals, OFF, ld, [0], output=output, fill=not output)
        (d.outputs if output else d.inputs)[name] = buf
        if output:
            d.masks[name] = mask
        return ld

    def vector(name, n, values=None):
        output = values is None
        buf, mask = _vector(torch.zeros(n, dtype=torch.float64) if output else values, VOFF, output=output,
                            fill=not output)
        (d.outputs if output else d.inputs)[name] = buf
        if output:
            d.masks[name] = mask
        d.at[name] = (name, VOFF)

    dqk_extra = c.qk_extra if c.dqk_extra < 0 else c.dqk_extra
    dv_extra = c.v_extra if c.dv_extra < 0 else c.dv_extra
    if c.shared_v:
        d.qk_ld = d.v_ld = matrix("qkv", 3 * C, c.qk_extra, torch.cat([p.q, p.k, p.v], 1))
        d.dqk_ld = d.dv_ld = matrix("dqkv", 3 * C, dqk_extra)
        d.at.update(q=("qkv", OFF), k=("qkv", OFF + C), v=("qkv", OFF + 2 * C),
                    dq=("dqkv", OFF), dk=("dqkv", OFF + C), dv=("dqkv", OFF + 2 * C))
        d.cols = dict(dq=("dqkv", 0), dk=("dqkv", C), dv=("dqkv", 2 * C))
    else:
        d.qk_ld = matrix("qk", 2 * C, c.qk_extra, torch.cat([p.q, p.k], 1))
        d.v_ld = matrix("v", C, c.v_extra, p.v)
        d.dqk_ld = matrix("dqk", 2 * C, dqk_extra)
        d.dv_ld = matrix("dv", C, dv_extra)
        d.at.update(q=("qk", OFF), k=("qk", OFF + C), v=("v", OFF), dq=("dqk", OFF), dk=("dqk", OFF + C),
                    dv=("dv", OFF))
        d.cols = dict(dq=("dqk", 0), dk=("dqk", C), dv=("dv", 0))
    d.out_ld = matrix("out", C, c.out_extra)
    matrix("dout", C, c.out_extra, p.dout)
    d.at.update(out=("out", OFF), dout=("dout", OFF))
    d.cols["out"] = ("out", 0)
    d.lds = dict(out=d.out_ld, dq=d.dqk_ld, dk=d.dqk_ld, dv=d.dv_ld)
    for name in ("q_pad", "k_pad", "v_pad"):
        if getattr(p, name) is not None:
            vector(name, C, getattr(p, name))
    vector("rpb_table", R.T * c.heads, p.rpb.reshape(-1))
    vector("lse", p.ref["geom"].nwin * c.heads * R.N)
    vector("d_rpb_table", R.T * c.heads)
    for name in ("dq_pad", "dk_pad", "dv_pad"):
        if getattr(c, name):
            vector(name, C)
    if c.live is not None:
        d.inputs["sample_live"] = torch.tensor(c.live, dtype=torch.float32)
        d.at["sample_live"] = ("sample_live", 0)
        dead = p.dead_rows
        for name, (alloc, off) in (("q", d.at["q"]), ("k", d.at["k"]), ("v", d.at["v"]), ("dout", d.at["dout"])):
            ld = d.qk_ld if name in "qk" else (d.v_ld if name == "v" else d.out_ld)
            torch.as_strided(d.inputs[alloc], (rows, C), (ld, 1), off)[dead] = float("nan")
    return d


def owned(d, name, buf):
    """The [rows, C] view of row output `name` inside allocation `buf` (any device)."""
    alloc, col = d.cols[name]
    return torch.as_strided(buf, (d.case.rows, d.case.C), (d.lds[name], 1), OFF + col)


# ---------------------------------------------------------------------------------------------
# The cases
# ---------------------------------------------------------------------------------------------
GEOMETRIES = [(7, 7, 0), (7, 7, 3), (14, 21, 3), (1, 1, 0), (1, 1, 3), (3, 20, 1), (8, 6, 6), (13, 15, 3), (10, 12, 3),
              (9, 16, 2)]
OCCUPANCIES = [(1, 1), (1, 3), (3, 1), (2, 3), (1, 5), (2, 2)]
# (geometry, occupancy) pairs of the sweep; MIXED holds fast-path and slow-path windows in one launch
GEOMETRY_PAIRS = [((7, 7, 0), (1, 1)), ((1, 1, 0), (1, 1)), ((1, 1, 3), (1, 3)), ((7, 7, 3), (3, 1)),
                  ((14, 21, 3), (1, 3)), ((3, 20, 1), (2, 3)), ((8, 6, 6), (1, 5)), ((13, 15, 3), (2, 2)),
                  ((10, 12, 3), (1, 5)), ((9, 16, 2), (2, 3)), ((9, 16, 2), (1, 3)), ((3, 20, 1), (1, 3)),
                  ((3, 20, 1), (1, 5)), ((7, 7, 0), (2, 3)), ((14, 21, 3), (2, 2))]
MIXED = "13x15s3-B2h2"


def _name(geo, occ):
    return f"{geo[0]}x{geo[1]}s{geo[2]}-B{occ[0]}h{occ[1]}"


def nitems(case):
    return case.B * ((case.H + 6) // 7) * ((case.W + 6) // 7) * case.heads


def geometry_cases():
    """Geometry x occupancy: nwin * heads % 4 takes each of 0..3 at least twice (workgroups of 4
    waves, one (window, head) item each), one case is a single item on a single token, and MIXED
    holds windows with and without pad tokens (both backward paths in one launch)."""
    assert all(g in GEOMETRIES and o in OCCUPANCIES for g, o in GEOMETRY_PAIRS)
    assert {g for g, _ in GEOMETRY_PAIRS} == set(GEOMETRIES) and {o for _, o in GEOMETRY_PAIRS} == set(OCCUPANCIES)
    cases = [Case(name=_name(g, o), H=g[0], W=g[1], shift=g[2], B=o[0], heads=o[1], seed=i)
             for i, (g, o) in enumerate(GEOMETRY_PAIRS)]
    rem = Counter(nitems(c) % 4 for c in cases)
    assert all(rem[r] >= 2 for r in range(4)), rem
    assert any(nitems(c) % 4 == 1 and c.rows == 1 for c in cases)
    pads = problem(next(c for c in cases if c.name == MIXED)).ref["geom"].row.lt(0).any(1)
    assert pads.any().item() and not pads.all().item()
    return cases


LAYOUT_GEOMETRIES = {"pads-mask": dict(H=10, W=12, shift=3, B=2, heads=3), "plain": dict(H=7, W=14, shift=0, B=2, heads=2)}

LAYOUTS = {
    "swin": dict(),
    "crf": dict(shared_v=False, v_pad=False),
    "sepv-vpad": dict(shared_v=False),
    "qpad-only": dict(k_pad=False),
    "kpad-only": dict(q_pad=False),
    "no-pads": dict(q_pad=False, k_pad=False, v_pad=False),
    "wide-ld": dict(shared_v=False, v_pad=False, qk_extra=8, v_extra=4),
    "wide-ld-shared": dict(qk_extra=12),
    "out-ld": dict(out_extra=4),
    "dqk-ld": dict(shared_v=False, v_pad=False, dqk_extra=8),
    "dqkv-ld-shared": dict(dqk_extra=4),
    "dv-ld": dict(shared_v=False, dv_extra=12),
    "no-dq_pad": dict(dq_pad=False),
    "no-dk_pad": dict(dk_pad=False),
    "no-dv_pad": dict(dv_pad=False),
    "no-dpads": dict(dq_pad=False, dk_pad=False, dv_pad=False),
}


def layout_cases():
    return [Case(name=f"{gname}-{lname}", seed=100 + gi, **geo, **lay)
            for gi, (gname, geo) in enumerate(LAYOUT_GEOMETRIES.items()) for lname, lay in LAYOUTS.items()]


# one relative offset (query - key) per geometry, heads = 3; tests/test_winattn_contract_ref.py
# asserts the share of exact queries each gives.  The single query of the 1x1 grid is exact too:
# at (-1, -1) its key is the pad token (1, 1), so its out row is v_pad.
GATHER = [((14, 21, 3), (0, 1)), ((13, 15, 3), (1, 0)), ((3, 20, 1), (-1, -1)), ((1, 1, 0), (-1, -1))]
GATHER_EXACT_P = 1 - 1e-30


def gather_cases():
    return [Case(name=f"gather-{g[0]}x{g[1]}s{g[2]}-d{o[0]}_{o[1]}", H=g[0], W=g[1], shift=g[2], B=1, heads=3, gather=o,
                 seed=200 + i) for i, (g, o) in enumerate(GATHER)]


def gather_expected(case):
    """exact [rows] bool and want [rows, C] float32: the real queries whose reference attention
    row has a maximum probability >= 1 - 1e-30 in every head, and the v row or pad vector the
    reference gathers for them."""
    p = problem(case)
    geom, P = p.ref["geom"], p.ref["P"]                     # P [nwin, heads, q, key]
    pmax, key = P.max(-1)
    sure = (pmax >= GATHER_EXACT_P).all(1)                  # [nwin, q]
    assert (key == key[:, :1])[sure[:, None].expand_as(key)].all().item()   # every head picks the same key
    key = key[:, 0]                                         # [nwin, q]
    src = torch.gather(geom.row, 1, key)                    # row the picked key reads, -1: pad vector
    vpad = p.v_pad if p.v_pad is not None else torch.zeros(case.C, dtype=torch.float64)
    picked = torch.where((src >= 0)[:, :, None], p.v[src.clamp(min=0)], vpad.view(1, 1, -1))
    real = geom.row >= 0
    exact = torch.zeros(case.rows, dtype=torch.bool)
    exact[geom.row[real]] = sure[real]
    want = torch.zeros(case.rows, case.C, dtype=torch.float64)
    want[geom.row[real]] = picked[real]
    per_window = [(sure[w] & real[w]).any().item() for w in range(geom.nwin)]
    return exact, want.float(), per_window


DEAD = Case(name="dead0-7x7s0-B3h3", H=7, W=7, shift=0, B=3, heads=3, live=(0.0, 1.0, 1.0), seed=300)


def all_cases():
    return geometry_cases() + layout_cases() + gather_cases() + [DEAD]
