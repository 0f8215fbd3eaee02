"""The train-mode ComplexBatchNormal + PReLU kernels -- idv_cbn_stats, idv_cbn_finalize, idv_cbn_fold, idv_cbn_apply_prelu, _to,
_to_img, idv_cbn_bwd_reduce, idv_cbn_bwd_finalize, idv_cbn_bwd_apply, _img, idv_cconv2d_bwd_bias and the replica collapse behind
the conv epilogues' moment sums -- against the float64 reference of tests/cbn_ref.py (itself checked on the CPU in
tests/test_cbn_ref_host.py).  Every entry is called through the C ABI on buffers the test lays out itself (slack in front and
behind, the pitch Jp and Tp of the case), and judged per channel or per element, never over a whole tensor.  Inputs are `exact`
(integers in [-3, 3], Z entries in {+-2, +-1, +-1/2, 0}, slope 1/4: every value and sum is exact in fp32 and in any order) or
`normal`; the reference is evaluated at the fp32 values the device sees.

Bounds, u = 2^-24.
  derived   exact kind: every bit equal (sums: every double equal).
            idv_cbn_stats, idv_cbn_bwd_reduce: double accumulation of fp32 values, n 2^-53 sum |term| for n terms; the slope
            sum adds the fp32 rounding of u, 3 u (|Zrr y_r| + |Zri y_i| + |s_r|) |dz| per element.
            idv_cbn_finalize moments: double arithmetic rounded once, then + eps in fp32: 2 u (|V| + mean^2) for the variances,
            u |mean| for the means; the running buffers copy these bits on a first call, and a later call adds the rounding of
            momentum, two products and a sum: 4 u (|momentum old| + |(1 - momentum) new|).
            idv_cbn_apply_prelu, _to, _to_img: 4 u (|Zrr y_r| + |Zri y_i| + |s_r|) per element, times the slope below zero (two
            products and two sums that the compiler may fuse, and the slope product).  idv_cbn_bwd_apply, _img: 8 u sum |terms|
            of the nine-term expression.  idv_cconv2d_bwd_bias: a double sum rounded once, u |ref|.
            The split image: hi + lo within 2^-16 of the planar result; exact kind: hi holds the value, lo is 0.
  measured  the fold of idv_cbn_finalize and idv_cbn_fold, every output of idv_cbn_bwd_finalize, the distance between the Z of
            the two finalize kernels, and the chain stats -> finalize -> apply -> reduce -> finalize -> apply against autograd:
            min(cap, 4 x the worst measured on the MI355X with the cap as the bound), cap = TOL = 2e-5 for forward values and
            GTOL = 2e-4 for gradients, relative to the largest reference magnitude of the channel (of the (channel, bin row)
            block for dy; of the group Z / A / c / mu within coef, which differ by orders of magnitude).  MEASURED below,
            DESIGN.md 3.5.2.  The worst channel or block of every call is printed.

Layout and reads.  Outputs are pre-filled with a sentinel and, in a second call, with another: what is written must come out
with the same bits.  Guard columns tp == 0 and T < tp < Tp of the out-of-place results are +0.0, the in-place entry leaves them
untouched; pitch columns [B Tp, Jp), rows behind the last plane and both slacks keep their sentinel.  Inputs carry 7.0 in guard and
pitch columns; a call with NaN there and in the slacks returns the same bits.

Degenerate channels (constant, or imag == real) are outside the conditions the bounds rest on: test_degenerate_channels_stay_finite
asserts finite outputs and prints the errors (fold of idv_cbn_finalize at imag == real: 1.3e-3 of the channel's largest entry, the
fp32 cancellation of Vrr Vii - Vri^2; every other output below 4e-8).

Corrections these tests led to: idv_cbn_stats, idv_cbn_apply_prelu, idv_cbn_apply_prelu_to, idv_cbn_bwd_reduce
and idv_cbn_bwd_apply accepted Jp < B Tp (rows overlap or run past the buffer), Tp < t_valid + 1 and t_valid < 1; the image twins
the last two.  All are IDV_EINVAL now, and a refused call writes nothing."""
import pytest
import torch

import cbn_ref as R

pytestmark = pytest.mark.gpu
TOL, GTOL = 2e-5, 2e-4       # the project's caps for forward values and for gradients
U = 2.0 ** -24
ONE = 1 + 1e-6               # room for the second-order terms of a derived bound
SENT = (-12345.0, 54321.0)
SENT16 = (0x5A5A, 0x3C3C)
BEHIND, FILL, GAP = 2, 7.0, 128
NAN = float("nan")
# The worst channel (block) measured on the MI355X with the caps as bounds, per entry and kind: the largest error over the largest
# reference magnitude of the channel.  The asserted bound is min(cap, 4 x this).
MEASURED = {
    ("finalize_fold", "normal"): 5.25e-07, ("fold", "normal"): 4.58e-07, ("z_distance", "normal"): 2.67e-07,
    # double arithmetic rounded once: about u; mu is copied
    ("bwd_finalize_coef_Z", "normal"): 5.53e-08, ("bwd_finalize_coef_A", "normal"): 5.39e-08, ("bwd_finalize_coef_c", "normal"): 5.72e-08,
    ("bwd_finalize_coef_mu", "normal"): 0.0, ("bwd_finalize_dgamma_rr", "normal"): 5.28e-08, ("bwd_finalize_dgamma_ri", "normal"): 5.85e-08,
    ("bwd_finalize_dgamma_ii", "normal"): 5.28e-08, ("bwd_finalize_dbeta_r", "normal"): 5.42e-08, ("bwd_finalize_dbeta_i", "normal"): 5.41e-08,
    ("bwd_finalize_dslope", "normal"): 4.85e-08,
    ("chain_z", "normal"): 2.13e-07, ("chain_dy", "normal"): 1.16e-07, ("chain_dgamma_rr", "normal"): 1.54e-07,
    ("chain_dgamma_ri", "normal"): 3.18e-07, ("chain_dgamma_ii", "normal"): 2.90e-07, ("chain_dbeta_r", "normal"): 5.24e-08,
    ("chain_dbeta_i", "normal"): 2.94e-08, ("chain_dslope", "normal"): 3.75e-08,
}
MISSED = []
GRADS = ("dgamma_rr", "dgamma_ri", "dgamma_ii", "dbeta_r", "dbeta_i")
COEF_GROUPS = (("Z", 0, 4), ("A", 4, 7), ("c", 7, 9), ("mu", 9, 11))


@pytest.fixture(autouse=True)
def no_missed_bound_left_over():
    MISSED.clear()


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def judge(entry, kind, cap, what, got, want, dims):
    """Print the worst channel / block of one call and hold it to the entry's bound; a miss is raised by settle()."""
    err, k = R.worst(got, want, dims)
    m = MEASURED.get((entry, kind))
    b = cap if m is None else min(cap, 4 * m)
    print(f"CBN-MEASURE\t{entry}\t{kind}\t{err:.3e}\t{what} (worst at {k}, bound {b:.3e})")
    if not (err < b or err == 0):
        MISSED.append(f"{entry} {kind} {what}: {err:.3e} at {k} against {b:.3e}")


def settle():
    assert not MISSED, "; ".join(MISSED)


# ----------------------------------------------------------------------------- buffers
class Buf:
    """n elements with `slack` elements in front and behind, all filled with `fill`."""

    def __init__(self, ops, n, fill, dtype=torch.float32, v=None, slack=None):
        slack = ops.SLACK if slack is None else slack
        self.ops, self.n, self.off, self.fill = ops, n, slack, fill
        self.flat = torch.full((n + 2 * slack,), fill, dtype=dtype, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.body = self.flat[slack:slack + n]
        if v is not None:
            self.body[:] = v.reshape(-1).to(self.flat)

    def ptr(self):
        return self.ops.L._P(self.body.data_ptr())

    def bits(self):
        return self.flat.view(torch.int64 if self.flat.dtype == torch.float64 else torch.int32)

    def written(self):
        return self.body.view(torch.int64 if self.flat.dtype == torch.float64 else torch.int32)

    def untouched(self):
        return bool((self.flat == self.fill).all())

    def check(self, what):
        assert bool((self.flat[:self.off] == self.fill).all()) and bool((self.flat[self.off + self.n:] == self.fill).all()), \
            f"{what}: written outside its {self.n} elements"

    def poison(self):
        self.flat[:self.off] = NAN
        self.flat[self.off + self.n:] = NAN


class Planes(Buf):
    """Planar [2 C F + BEHIND rows][Jp]: v [2, C, F, B, T] on the kept columns, `fill` everywhere else.  guards: what check()
    expects in the guard columns -- "zero" (+0.0) or "fill" (untouched)."""

    def __init__(self, ops, g, fill, v=None, guards="zero"):
        self.C, self.F, self.B, self.T, self.Tp, self.Jp = g
        self.rows, self.J, self.guards = 2 * self.C * self.F, self.B * self.Tp, guards
        assert self.Jp >= self.J and self.Tp >= self.T + 1
        super().__init__(ops, (self.rows + BEHIND) * self.Jp, fill)
        self.plane = self.body.view(self.rows + BEHIND, self.Jp)
        if v is not None:
            R.place(self.plane, v.float().cuda(), self.Tp)

    def mask(self):
        return R.guard_mask(self.B, self.T, self.Tp, "cuda")

    def kept(self):
        return R.read(self.plane, self.C, self.F, self.B, self.T, self.Tp).cpu()

    def full(self):
        """[2, C, F, Jp]"""
        return self.plane[:self.rows].view(2, self.C, self.F, self.Jp)

    def written(self):
        return self.plane[:self.rows, :self.J][:, ~self.mask()].contiguous().view(torch.int32)

    def check(self, what):
        g = self.plane[:self.rows, :self.J][:, self.mask()]
        if self.guards == "zero":
            assert bool((g == 0).all()) and not bool(torch.signbit(g).any()), f"{what}: a guard column (tp == 0 or tp > T) is not +0.0"
        else:
            assert bool((g == self.fill).all()), f"{what}: a guard column was written"
        assert bool((self.plane[:self.rows, self.J:] == self.fill).all()), f"{what}: the pitch columns [B Tp, Jp) were written"
        assert bool((self.plane[self.rows:] == self.fill).all()), f"{what}: rows behind the last plane were written"
        super().check(what)

    def poison(self):
        super().poison()
        self.plane[:self.rows, :self.J][:, self.mask()] = NAN
        self.plane[:self.rows, self.J:] = NAN
        self.plane[self.rows:] = NAN


class Img:
    """The split image of an activation with C % 4 == 0: C / 4 octets x F rows x Jp slots of 8 bf16 (re, im of 4 channels), a hi
    and a lo plane lo_off apart, GAP halfwords of sentinel in front of, between (twice) and behind them."""

    def __init__(self, ops, g, fill):
        self.ops, self.fill = ops, fill
        self.C, self.F, self.B, self.T, self.Tp, self.Jp = g
        self.n = self.C // 4 * self.F * self.Jp * 8
        self.lo_off = self.n + 2 * GAP
        self.flat = torch.full((GAP + self.lo_off + self.n + GAP,), fill, dtype=torch.int16, device="cuda")
        assert self.flat.data_ptr() % 16 == 0

    def ptr(self, shift=0):
        return self.ops.L._P(self.flat.data_ptr() + 2 * (GAP + shift))

    def bits(self):
        return self.flat

    def written(self):
        return torch.stack([self.flat[o:o + self.n] for o in (GAP, GAP + self.lo_off)])

    def untouched(self):
        return bool((self.flat == self.fill).all())

    def values(self, o):
        """One plane as fp32 [2, C, F, Jp]."""
        v = (self.flat[o:o + self.n].to(torch.int32) << 16).view(torch.float32)
        return v.view(self.C // 4, self.F, self.Jp, 4, 2).permute(4, 0, 3, 1, 2).reshape(2, self.C, self.F, self.Jp)

    def check(self, what):
        for o in (GAP, GAP + self.lo_off):
            f = self.flat
            assert bool((f[o - 64:o - 56] == 0).all()), f"{what}: the zero slot in front of a plane is not zero"
            assert bool((f[o + self.n:o + self.n + 64] == 0).all()), f"{what}: the 8 slots behind a plane are not zero"
            assert bool((f[o - GAP:o - 64] == self.fill).all()) and bool((f[o - 56:o] == self.fill).all()) and \
                bool((f[o + self.n + 64:o + self.n + GAP] == self.fill).all()), f"{what}: written outside the planes and their edge slots"

    def matches(self, planar, exact, what):
        """planar: the Planes the same call wrote.  Every slot hi + lo reproduces it within 2^-16, guard and pitch slots are 0."""
        hi, lo = self.values(GAP), self.values(GAP + self.lo_off)
        J = planar.J
        want = planar.full().clone()
        want[..., J:] = 0
        assert bool((hi[..., J:] == 0).all()) and bool((lo[..., J:] == 0).all()), f"{what}: a pitch slot [B Tp, Jp) of the image is not zero"
        g = planar.mask()
        assert bool((hi[..., :J][..., g] == 0).all()) and bool((lo[..., :J][..., g] == 0).all()), f"{what}: a guard slot of the image is not zero"
        assert bool(((hi.double() + lo.double() - want.double()).abs() <= 2.0 ** -16 * want.double().abs()).all()), \
            f"{what}: hi + lo is further than 2^-16 from the planar result"
        if exact:
            assert torch.equal(hi, want) and bool((lo == 0).all()), f"{what}: hi does not hold the exact value"


def geo(case):
    return (case.C, case.F, case.B, case.T, case.Tp, case.Jp)


def run(launch, make):
    """make(k) -> the outputs of one call, pre-filled with sentinel k; launch(outputs) calls the entry.  Two calls on the two
    sentinels -> the outputs of the first, after the layout checks on both and the comparison of what they wrote."""
    a, b = make(0), make(1)
    launch(a)
    launch(b)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        x.check("first call")
        y.check("second call")
        assert torch.equal(x.written(), y.written()), "an element is left unwritten, or a second call differs"
    return a


def rerun(launch, make, first, why):
    c = make(0)
    launch(c)
    torch.cuda.synchronize()
    assert all(torch.equal(x.bits(), y.bits()) for x, y in zip(first, c)), why


READS = "guard columns, pitch columns, rows behind the last plane or a slack of an input reach the result"


def same_f32(got, want):
    """Every bit equal (want: float64 holding fp32 values)."""
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.float().contiguous().view(torch.int32))


def within(got, want, room):
    return bool(((got.cpu().double() - want).abs() <= room * ONE).all())


def dev32(t):
    return t.float().cuda().contiguous()


def inputs(ops, case, salt=0):
    """The case's draw with every tensor rounded to fp32 (what the device sees), as float64, plus the device operands."""
    d = R.draw(case, salt)
    d["y"], d["dz"] = d["y"].float().double(), d["dz"].float().double()
    if case.kind == "normal":
        d["gam"] = tuple(g.float().double() for g in d["gam"])
        d["beta"] = tuple(b.float().double() for b in d["beta"])
        m, _, fo = R.finalize(R.moment_sums(d["y"]), case.count, d["gam"], d["beta"])
        d["moments"], d["fold"] = m.float().double(), fo.float().double()
    d["slope_t"] = None if case.slope is None else torch.full((1,), case.slope, device="cuda")
    d["fold_t"] = dev32(d["fold"])
    return d


def call(ops, name, *args):
    L = ops.L
    ops.call(name, *[L.p(None) if a is None else (a.ptr() if isinstance(a, (Buf, Img)) else (L.p(a) if torch.is_tensor(a) else
                                                                                              (L.i(a) if isinstance(a, int) else a)))
                     for a in args], L.stream_ptr())


def u_terms(y, fo):
    """sum of the magnitudes of the three terms of u, [2, C, F, B, T]."""
    yr, yi = y[0].abs(), y[1].abs()
    a = lambda k: R._col(fo, k).abs()
    return torch.stack((a(0) * yr + a(1) * yi + a(4), a(2) * yr + a(3) * yi + a(5)))


ELEMENTWISE = [c for c in R.CASES if c.name != "e_cap16"]


def with_entries(entries, img):
    """(case, entry) pairs: the image twin takes C % 4 == 0 only (refused otherwise: test_refusals)."""
    pairs = [(c, e) for c in ELEMENTWISE for e in entries if e != img or c.C % 4 == 0]
    return dict(argvalues=pairs, ids=[f"{c.name}-{e}" for c, e in pairs])


SUMS = [c for c in R.CASES if not c.name.startswith("e_cap64")]
ids = lambda cases: [c.name for c in cases]


# ----------------------------------------------------------------------------- idv_cbn_stats
@pytest.mark.parametrize("case", SUMS, ids=ids(SUMS))
def test_stats(ops, case):
    d = inputs(ops, case)
    y = Planes(ops, geo(case), FILL, d["y"])
    before = y.flat.clone()
    pre = 3.0                                     # the entry adds to what stats holds
    st = Buf(ops, 5 * case.C, pre, torch.float64, slack=16)
    st_nan = Buf(ops, 5 * case.C, pre, torch.float64, slack=16)
    call(ops, "idv_cbn_stats", y, case.C, case.F, case.B, case.Tp, case.Jp, case.T, st)
    y.poison()
    call(ops, "idv_cbn_stats", y, case.C, case.F, case.B, case.Tp, case.Jp, case.T, st_nan)
    torch.cuda.synchronize()
    st.check("stats")
    want = R.moment_sums(d["y"]) + pre
    for got in (st, st_nan):
        g = got.body.view(case.C, 5).cpu()
        if case.kind == "exact":
            assert torch.equal(g, want), (g, want)
        else:
            r, i = d["y"][0].abs(), d["y"][1].abs()
            mag = torch.stack([t.sum(dim=(1, 2, 3)) for t in (r, i, r * r, i * i, r * i)], dim=1)
            assert within(g, want, (case.count * mag + want.abs()) * 2.0 ** -53), "a moment sum is off by more than double accumulation allows"
    assert torch.equal(before[y.off:y.off + y.n].view(-1, y.Jp)[:y.rows, :y.J][:, ~y.mask()], y.plane[:y.rows, :y.J][:, ~y.mask()]), \
        "the input was written"


def test_conv_moment_sums_through_the_replicas(ops):
    """idv_cconv2d_fwd with stats_work / stats_rep = 4: the collapsed [Cout][5] are the sums of the conv's float64 output, and
    the same doubles as without replicas."""
    c, d = R.CONV, R.draw_conv()
    cin, cout, F, T, B = c["cin"], c["cout"], c["F"], c["T"], c["B"]
    Tp, Fo = T + 1, (F - 1) // 2 + 1
    Jp = (B * Tp + 3) // 4 * 4
    assert ops.L.lib().idv_cconv_config(0, cin, cout, F) > 0
    x = Planes(ops, (cin, F, B, T, Tp, Jp), 0.0, d["x"])
    wfrag, bias = ops.pack_cconv(*(dev32(d[k]) for k in ("w_re", "w_im", "b_re", "b_im")), None)
    want_y = R.cconv(d["x"], d["w_re"], d["w_im"], d["b_re"], d["b_im"])
    want = R.moment_sums(want_y)
    got = []
    for rep in (4, 0):
        out = Planes(ops, (cout, Fo, B, T, Tp, Jp), SENT[0])
        st = Buf(ops, 5 * cout, 0.0, torch.float64, slack=16)
        work = Buf(ops, max(rep, 1) * 5 * cout, 0.0, torch.float64, slack=16)
        call(ops, "idv_cconv2d_fwd", x, cin, None, 0, 0, 1, wfrag, bias, None, out, st, work if rep else None, rep, 0, -1, cout, F, B, Tp,
             Jp, T)
        torch.cuda.synchronize()
        st.check("stats")
        work.check("stats_work")
        assert same_f32(out.kept(), want_y), "the conv's own output is not the exact integer result"
        got.append(st.body.view(cout, 5).cpu())
        assert torch.equal(got[-1], want), (rep, got[-1], want)
        if rep:
            assert torch.equal(work.body.view(rep, cout, 5).sum(0).cpu(), want)
    assert torch.equal(got[0], got[1])


# ----------------------------------------------------------------------------- idv_cbn_finalize, idv_cbn_fold
def finalize_args(case, sums, p, first, momentum, run, moments, fold):
    return ("idv_cbn_finalize", sums, p.d(float(case.count)), *p.gam, *p.beta, case.C, 1 if first else 0, p.f(momentum), *run, moments, fold)


class Params:
    def __init__(self, ops, d):
        self.d, self.f = ops.L.d, ops.L.f
        self.gam, self.beta = [dev32(g) for g in d["gam"]], [dev32(b) for b in d["beta"]]


def moments_room(m):
    """The derived bound of the moments [5][C]."""
    sq = torch.stack((m[0] * 0, m[1] * 0, m[0] ** 2, (m[0] * m[1]).abs(), m[1] ** 2))
    f = torch.tensor([1.0, 1.0, 2.0, 2.0, 2.0], dtype=torch.float64).view(5, 1)
    return f * U * (m.abs() + sq)


FIN = R.FINALIZE_CASES + [R.BY_NAME[R.CHAIN]]


@pytest.mark.parametrize("momentum", [0.9, 0.5])
@pytest.mark.parametrize("case", FIN, ids=ids(FIN))
def test_finalize(ops, case, momentum):
    C = case.C
    d, d2 = inputs(ops, case), inputs(ops, case, 1)
    p = Params(ops, d)
    sums = [R.moment_sums(x["y"]).cuda() for x in (d, d2)]
    m_dev = float(torch.tensor(momentum, dtype=torch.float32))
    m1, run1, fo1 = R.finalize(sums[0].cpu(), case.count, d["gam"], d["beta"])
    # the blend is judged at the fp32 momentum the entry receives; 1 - momentum is exact in fp32 for 0.5 <= momentum <= 1
    m2, run2, fo2 = R.finalize(sums[1].cpu(), case.count, d["gam"], d["beta"], running=run1, momentum=m_dev)

    def make(k):
        return [Buf(ops, C, SENT[k]) for _ in range(5)] + [Buf(ops, 5 * C, SENT[k]), Buf(ops, 6 * C, SENT[k])]

    def first(o):
        call(ops, *finalize_args(case, sums[0], p, True, momentum, o[:5], o[5], o[6]))

    def both(o):
        first(o)
        call(ops, *finalize_args(case, sums[1], p, False, momentum, o[:5], o[5], o[6]))

    a = run(first, make)
    mom, fo = a[5].body.view(5, C).cpu(), a[6].body.view(C, 6).cpu()
    assert within(mom, m1, moments_room(m1)), "a batch moment is further from the float64 value than one rounding (and + eps) allows"
    for k in range(5):
        assert torch.equal(a[k].body.cpu(), mom[k]), "the first call does not copy the batch moments into the running buffers"
    judge("finalize_fold", case.kind, TOL, case.name, fo, fo1, (1,))
    b = run(both, make)
    mom_b, fo_b = b[5].body.view(5, C).cpu(), b[6].body.view(C, 6).cpu()
    assert within(mom_b, m2, moments_room(m2))
    judge("finalize_fold", case.kind, TOL, case.name + " second call", fo_b, fo2, (1,))
    got_run = torch.stack([b[k].body.cpu() for k in range(5)])
    room = m_dev * moments_room(m1) + (1 - m_dev) * moments_room(m2) + 4 * U * ((m_dev * run1).abs() + ((1 - m_dev) * m2).abs())
    assert within(got_run, run2, room), ("a running buffer is not momentum old + (1 - momentum) new", momentum,
                                         float((got_run.double() - run2).abs().max()))
    # no running buffers: only moments and fold are written; moments = NULL is accepted
    o = make(0)
    call(ops, *finalize_args(case, sums[0], p, True, momentum, [None] + o[1:5], o[5], o[6]))
    o2 = make(0)
    call(ops, *finalize_args(case, sums[0], p, False, momentum, [None] * 5, None, o2[6]))
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o[:5] + o2[:6]), "written without being asked to"
    assert torch.equal(o[5].bits(), a[5].bits()) and torch.equal(o[6].bits(), a[6].bits()) and torch.equal(o2[6].bits(), a[6].bits())
    # refusals
    o = make(0)
    for args in (finalize_args(case, sums[0], p, True, momentum, o[:3] + [None] + o[4:5], o[5], o[6]),
                 finalize_args(case, sums[0], p, True, momentum, o[:1] + [None] * 4, o[5], o[6]),
                 finalize_args(case._replace(B=0), sums[0], p, True, momentum, o[:5], o[5], o[6]),
                 finalize_args(case._replace(B=-1), sums[0], p, True, momentum, o[:5], o[5], o[6])):
        with pytest.raises(ops.L.IdvError, match=r"status -1 "):
            call(ops, *args)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)
    settle()


@pytest.mark.parametrize("case", FIN, ids=ids(FIN))
def test_fold(ops, case):
    """idv_cbn_fold against the reference from the same fp32 moments."""
    d = inputs(ops, case)
    p = Params(ops, d)
    mom = dev32(d["moments"])
    a = run(lambda o: call(ops, "idv_cbn_fold", mom, *p.gam, *p.beta, case.C, o[0]), lambda k: [Buf(ops, 6 * case.C, SENT[k])])
    judge("fold", case.kind, TOL, case.name, a[0].body.view(case.C, 6), R.fold(d["moments"], d["gam"], d["beta"]), (1,))
    settle()


# ----------------------------------------------------------------------------- the forward apply entries
def apply_checks(case, d, got, what):
    want = R.apply(d["y"], d["fold"], case.slope)
    if case.kind == "exact":
        assert same_f32(got, want), f"{what}: an element differs from the exact result (the sign of a zero included)"
    else:
        u = R.pre_activation(d["y"], d["fold"])
        room = 4 * U * u_terms(d["y"], d["fold"]) * (1.0 if case.slope is None else torch.where(u >= 0, torch.ones_like(u), torch.full_like(u, case.slope)))
        assert within(got, want, room), f"{what}: an element is further off than 4 u sum |terms|"


@pytest.mark.parametrize("case,entry", **with_entries(("to", "to_img", "in_place"), "to_img"))
def test_apply_prelu(ops, case, entry):
    d = inputs(ops, case)
    g = geo(case)
    tail = (case.C, case.F, case.B, case.Tp, case.Jp, case.T)
    if entry == "in_place":
        def make(k):
            return [Planes(ops, g, SENT[k], d["y"], guards="fill")]

        def launch(o, poisoned=False):
            if poisoned:
                o[0].poison()
            call(ops, "idv_cbn_apply_prelu", o[0], d["fold_t"], d["slope_t"], *tail)

        a = run(launch, make)
        apply_checks(case, d, a[0].kept(), entry)
        c = make(0)
        launch(c, True)
        torch.cuda.synchronize()
        assert torch.equal(c[0].written(), a[0].written()), READS
        assert bool(torch.isnan(c[0].plane[:c[0].rows, :c[0].J][:, c[0].mask()]).all()), "a guard column was written"
        return
    y = Planes(ops, g, FILL, d["y"])

    def make(k):
        return [Planes(ops, g, SENT[k])] + ([Img(ops, g, SENT16[k])] if entry == "to_img" else [])

    def launch(o):
        if entry == "to":
            call(ops, "idv_cbn_apply_prelu_to", y, d["fold_t"], d["slope_t"], *tail, o[0])
        else:
            call(ops, "idv_cbn_apply_prelu_to_img", y, d["fold_t"], d["slope_t"], *tail, o[0], o[1], ops.L.ll(o[1].lo_off))

    a = run(launch, make)
    apply_checks(case, d, a[0].kept(), entry)
    if entry == "to_img":
        a[1].matches(a[0], case.kind == "exact", entry)
    y.poison()
    rerun(launch, make, a, READS)


# ----------------------------------------------------------------------------- idv_cbn_bwd_reduce
@pytest.mark.parametrize("case", SUMS, ids=ids(SUMS))
def test_bwd_reduce(ops, case):
    d = inputs(ops, case)
    y, dz = Planes(ops, geo(case), FILL, d["y"]), Planes(ops, geo(case), FILL, d["dz"])
    C = case.C

    def launch(o):
        call(ops, "idv_cbn_bwd_reduce", dz, y, d["fold_t"], d["slope_t"], C, case.F, case.B, case.Tp, case.Jp, case.T, o[0])

    outs = [[Buf(ops, 8 * C, SENT[k], torch.float64, slack=16)] for k in (0, 1, 0)]
    launch(outs[0])
    launch(outs[1])
    y.poison()
    dz.poison()
    launch(outs[2])
    torch.cuda.synchronize()
    want = R.bwd_sums(d["dz"], d["y"], d["fold"], case.slope)
    if case.kind == "normal":
        u = R.pre_activation(d["y"], d["fold"])
        du = R.du_of(d["dz"], u, case.slope).abs()
        ya = d["y"].abs()
        s = lambda t: t.sum(dim=(1, 2, 3))
        zero = torch.zeros(C, dtype=torch.float64)
        mag = [s(du[0]), s(du[1]), s(du[0] * ya[0]), s(du[0] * ya[1]), s(du[1] * ya[0]), s(du[1] * ya[1])]
        s6 = zero
        if case.slope is not None:
            neg = (u <= 0).double()
            s6 = s((neg * d["dz"].abs() * (2 * case.count * 2.0 ** -53 * u.abs() + 3 * U * u_terms(d["y"], d["fold"]))).sum(0))
        room = torch.stack([case.count * 2.0 ** -53 * m for m in mag] + [s6, zero], dim=1)
    for o in outs:
        o[0].check("sums")
        got = o[0].body.view(C, 8).cpu()
        assert bool((got[:, 7] == 0).all()), "slot 7 is not 0"
        if case.kind == "exact":
            assert torch.equal(got, want), (got, want)
        else:
            assert within(got, want, room), ("a sum is off by more than double accumulation allows", (got - want).abs().max(0))


# ----------------------------------------------------------------------------- idv_cbn_bwd_finalize
def device_forward(ops, case, d, p):
    """idv_cbn_finalize on the float64 sums of the case -> (moments, fold) device tensors."""
    mom, fo = torch.empty(5 * case.C, device="cuda"), torch.empty(6 * case.C, device="cuda")
    call(ops, *finalize_args(case, R.moment_sums(d["y"]).cuda(), p, True, 0.9, [None] * 5, mom, fo))
    return mom, fo


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("case", FIN, ids=ids(FIN))
def test_bwd_finalize(ops, case, scale):
    C = case.C
    d = inputs(ops, case)
    p = Params(ops, d)
    mom, fo = device_forward(ops, case, d, p)
    torch.cuda.synchronize()
    moments, fold = mom.view(5, C).cpu().double(), fo.view(C, 6).cpu().double()
    sums_ref = R.bwd_sums(d["dz"], d["y"], fold, case.slope)
    sums = sums_ref.cuda()
    want = R.bwd_finalize(sums_ref, case.count, moments, d["gam"], scale)

    def make(k):
        return [Buf(ops, 12 * C, SENT[k])] + [Buf(ops, C, SENT[k]) for _ in range(5)] + [Buf(ops, 1, SENT[k])]

    def launch(o, dslope=True):
        call(ops, "idv_cbn_bwd_finalize", sums, p.d(float(case.count)), mom, *p.gam, C, *o[:6], o[6] if dslope else None, p.f(scale))

    a = run(launch, make)
    coef = a[0].body.view(C, 12).cpu()
    assert bool((coef[:, 11] == 0).all()) and not bool(torch.signbit(coef[:, 11]).any()), "coef[.][11] is not 0"
    for name, lo, hi in COEF_GROUPS:
        judge("bwd_finalize_coef_" + name, case.kind, GTOL, f"{case.name} scale {scale}", coef[:, lo:hi], want["coef"][:, lo:hi], (1,))
    for k, name in enumerate(GRADS):
        judge("bwd_finalize_" + name, case.kind, GTOL, f"{case.name} scale {scale}", a[1 + k].body, want[name], ())
    judge("bwd_finalize_dslope", case.kind, GTOL, f"{case.name} scale {scale}", a[6].body, want["dslope"], ())
    # the Z of the two finalize kernels: fp32 there, double from the fp32 moments here
    judge("z_distance", case.kind, TOL, case.name, coef[:, :4], fold[:, :4], (1,))
    o = make(0)
    launch(o, dslope=False)
    torch.cuda.synchronize()
    assert o[6].untouched() and all(torch.equal(x.bits(), y.bits()) for x, y in zip(o[:6], a[:6]))
    o = make(0)
    for count in (0.0, -1.0):
        with pytest.raises(ops.L.IdvError, match=r"status -1 "):
            call(ops, "idv_cbn_bwd_finalize", sums, p.d(count), mom, *p.gam, C, *o, p.f(scale))
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)
    settle()


# ----------------------------------------------------------------------------- idv_cbn_bwd_apply, _img
@pytest.mark.parametrize("case,entry", **with_entries(("planar", "img"), "img"))
def test_bwd_apply(ops, case, entry):
    d = inputs(ops, case)
    g, C = geo(case), case.C
    tail = (C, case.F, case.B, case.Tp, case.Jp, case.T)
    y, dz = Planes(ops, g, FILL, d["y"]), Planes(ops, g, FILL, d["dz"])
    if case.kind == "exact":
        fold_t, coef_t, fold, coef = d["fold_t"], dev32(d["coef"]), d["fold"], d["coef"]
    else:
        # the device's own fold and coef, from its own sums
        p = Params(ops, d)
        mom, fold_t = device_forward(ops, case, d, p)
        sums, coef_t = torch.empty(8 * C, dtype=torch.float64, device="cuda"), torch.empty(12 * C, device="cuda")
        call(ops, "idv_cbn_bwd_reduce", dz, y, fold_t, d["slope_t"], *tail, sums)
        grads = [torch.empty(C, device="cuda") for _ in range(5)]
        call(ops, "idv_cbn_bwd_finalize", sums, p.d(float(case.count)), mom, *p.gam, C, coef_t, *grads, None, p.f(1.0))
        torch.cuda.synchronize()
        fold, coef = fold_t.view(C, 6).cpu().double(), coef_t.view(C, 12).cpu().double()
        assert float(R.pre_activation(d["y"], fold).abs().min()) > 1e-5      # no branch can differ between fp32 and float64

    def make(k):
        return [Planes(ops, g, SENT[k])] + ([Img(ops, g, SENT16[k])] if entry == "img" else [])

    def launch(o):
        if entry == "planar":
            call(ops, "idv_cbn_bwd_apply", dz, y, fold_t, coef_t, d["slope_t"], *tail, o[0])
        else:
            call(ops, "idv_cbn_bwd_apply_img", dz, y, fold_t, coef_t, d["slope_t"], *tail, o[0], o[1], ops.L.ll(o[1].lo_off))

    a = run(launch, make)
    got, want = a[0].kept(), R.bwd_apply(d["dz"], d["y"], fold, coef, case.slope)
    if case.kind == "exact":
        assert same_f32(got, want), "an element differs from the exact result"
    else:
        tr, ti = R.bwd_terms(d["dz"], d["y"], fold, coef, case.slope)
        room = 8 * U * torch.stack((sum(t.abs() for t in tr), sum(t.abs() for t in ti)))
        assert within(got, want, room), "an element is further off than 8 u sum |terms|"
    if entry == "img":
        a[1].matches(a[0], case.kind == "exact", entry)
    y.poison()
    dz.poison()
    rerun(launch, make, a, READS)


# ----------------------------------------------------------------------------- idv_cconv2d_bwd_bias
@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("C", [5, 70])
def test_bias_grad(ops, C, kind):
    g = torch.Generator().manual_seed(C)
    sums = torch.randint(-2 ** 20, 2 ** 20, (C, 5), generator=g).double()
    if kind == "normal":
        sums = sums + torch.rand(C, 5, generator=g, dtype=torch.float64)
    s = sums.cuda()
    a = run(lambda o: call(ops, "idv_cconv2d_bwd_bias", s, C, o[0], o[1]), lambda k: [Buf(ops, C, SENT[k]), Buf(ops, C, SENT[k])])
    for got, want in zip(a, R.bias_grad(sums)):
        if kind == "exact":
            assert same_f32(got.body, want)
        else:
            assert within(got.body, want, U * want.abs())


# ----------------------------------------------------------------------------- the chain
def test_chain_against_autograd(ops):
    """stats -> finalize -> apply_to -> bwd_reduce -> bwd_finalize -> bwd_apply on device buffers, every result against torch
    autograd in float64 through the reference's forward."""
    case = R.BY_NAME[R.CHAIN]
    d = inputs(ops, case)
    p = Params(ops, d)
    g, C = geo(case), case.C
    tail = (C, case.F, case.B, case.Tp, case.Jp, case.T)
    y, dz = Planes(ops, g, FILL, d["y"]), Planes(ops, g, FILL, d["dz"])
    z, dy = Planes(ops, g, SENT[0]), Planes(ops, g, SENT[0])
    st = torch.zeros(5 * C, dtype=torch.float64, device="cuda")
    mom, fo, coef = torch.empty(5 * C, device="cuda"), torch.empty(6 * C, device="cuda"), torch.empty(12 * C, device="cuda")
    sums = torch.empty(8 * C, dtype=torch.float64, device="cuda")
    grads = [torch.empty(C, device="cuda") for _ in range(5)]
    dslope = torch.zeros(1, device="cuda")
    call(ops, "idv_cbn_stats", y, *tail, st)
    call(ops, *finalize_args(case, st, p, True, 0.9, [None] * 5, mom, fo))
    call(ops, "idv_cbn_apply_prelu_to", y, fo, d["slope_t"], *tail, z)
    call(ops, "idv_cbn_bwd_reduce", dz, y, fo, d["slope_t"], *tail, sums)
    call(ops, "idv_cbn_bwd_finalize", sums, p.d(float(case.count)), mom, *p.gam, C, coef, *grads, dslope, p.f(1.0))
    call(ops, "idv_cbn_bwd_apply", dz, y, fo, coef, d["slope_t"], *tail, dy)
    torch.cuda.synchronize()
    z.check("z")
    dy.check("dy")
    want = R.backward_autograd(d["y"], d["dz"], d["gam"], d["beta"], case.slope)
    _, _, fold = R.finalize(R.moment_sums(d["y"]), case.count, d["gam"], d["beta"])
    judge("chain_z", "normal", TOL, "per (channel, bin row)", z.kept().permute(1, 2, 0, 3, 4), R.apply(d["y"], fold, case.slope).permute(1, 2, 0, 3, 4), (2, 3, 4))
    judge("chain_dy", "normal", GTOL, "per (channel, bin row)", dy.kept().permute(1, 2, 0, 3, 4), want["dy"].permute(1, 2, 0, 3, 4), (2, 3, 4))
    for k, name in enumerate(GRADS):
        judge("chain_" + name, "normal", GTOL, "per channel", grads[k], want[name], ())
    judge("chain_dslope", "normal", GTOL, "", dslope, want["dslope"], ())
    settle()


def test_degenerate_channels_stay_finite(ops):
    """A constant channel (V = eps) and a channel with imag == real (a singular covariance), where eps and the 1e-8 clamp decide:
    outside the conditions every bound above rests on, so the errors are printed, not bounded; every output is finite."""
    C, n = 2, 48
    case = R.Case("degenerate", "normal", C, 1, 1, n, 1, 0, True, 0)
    d = inputs(ops, R.FINALIZE_CASES[0])
    gam, beta = tuple(g[:C] for g in d["gam"]), tuple(b[:C] for b in d["beta"])
    y = d["y"][:, :C].clone()
    y[0, 0], y[1, 0] = 1.5, 0.5
    y[1, 1] = y[0, 1]
    dz = d["dz"][:, :C]
    p = Params(ops, dict(gam=gam, beta=beta))
    mom, fo = device_forward(ops, case, dict(y=y), p)
    torch.cuda.synchronize()
    moments, fold = mom.view(5, C).cpu().double(), fo.view(C, 6).cpu().double()
    sums = R.bwd_sums(dz, y, fold, case.slope)
    outs = [torch.empty(12 * C, device="cuda")] + [torch.empty(C, device="cuda") for _ in range(5)] + [torch.empty(1, device="cuda")]
    call(ops, "idv_cbn_bwd_finalize", sums.cuda(), p.d(float(n)), mom, *p.gam, C, *outs, p.f(1.0))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in [mom, fo] + outs)
    _, _, fold_ref = R.finalize(R.moment_sums(y), n, gam, beta)
    want = R.bwd_finalize(sums, n, moments, gam)
    for name, got, ref in (("fold", fo.view(C, 6), fold_ref), ("coef", outs[0].view(C, 12), want["coef"])) + \
            tuple((k, outs[1 + i], want[k]) for i, k in enumerate(GRADS)):
        err = (got.cpu().double() - ref).abs().reshape(C, -1).amax(1) / ref.abs().reshape(C, -1).amax(1).clamp_min(1e-300)
        print(f"CBN-DEGENERATE\t{name}\tconstant {float(err[0]):.3e}\timag == real {float(err[1]):.3e}")


# ----------------------------------------------------------------------------- refusals
def test_refusals(ops):
    """Jp < B Tp, Tp < t_valid + 1 and t_valid < 1 are IDV_EINVAL at all seven planar entries, C % 4, lo_off_elems % 8 and a
    misaligned img at the image twins; a refused call writes nothing."""
    case = R.BY_NAME["e_c4"]
    d = inputs(ops, case)
    g, C = geo(case), case.C
    y, dz = Planes(ops, g, FILL, d["y"]), Planes(ops, g, FILL, d["dz"])
    out, img = Planes(ops, g, SENT[0]), Img(ops, g, SENT16[0])
    act = Planes(ops, g, SENT[0])
    st, sums = Buf(ops, 5 * C, SENT[0], torch.float64, slack=16), Buf(ops, 8 * C, SENT[0], torch.float64, slack=16)
    coef_t = dev32(d["coef"])
    fo, sl, L = d["fold_t"], d["slope_t"], ops.L
    good = dict(C=C, F=case.F, B=case.B, Tp=case.Tp, Jp=case.Jp, T=case.T)
    bad = [dict(Jp=case.B * case.Tp - 1), dict(Tp=case.T), dict(T=0), dict(T=-1), dict(T=case.Tp)]
    entries = {
        "idv_cbn_stats": lambda q, i: (y, *q, st),
        "idv_cbn_apply_prelu": lambda q, i: (act, fo, sl, *q),
        "idv_cbn_apply_prelu_to": lambda q, i: (y, fo, sl, *q, out),
        "idv_cbn_bwd_reduce": lambda q, i: (dz, y, fo, sl, *q, sums),
        "idv_cbn_bwd_apply": lambda q, i: (dz, y, fo, coef_t, sl, *q, out),
        "idv_cbn_apply_prelu_to_img": lambda q, i: (y, fo, sl, *q, out, i[0], L.ll(i[1])),
        "idv_cbn_bwd_apply_img": lambda q, i: (dz, y, fo, coef_t, sl, *q, out, i[0], L.ll(i[1])),
    }
    for name, args in entries.items():
        variants = [(dict(good, **kw), (img, img.lo_off)) for kw in bad]
        if name.endswith("_img"):
            variants += [(dict(good, C=C + 1), (img, img.lo_off)), (dict(good, C=2), (img, img.lo_off)), (good, (img, img.lo_off + 4)),
                         (good, (img.ptr(4), img.lo_off))]
        for q, i in variants:
            with pytest.raises(L.IdvError, match=r"status -1 "):
                call(ops, name, *args(tuple(q.values()), i))
    torch.cuda.synchronize()
    assert all(x.untouched() for x in (out, img, act, st, sums)), "a refused call wrote to its output"
