"""The kernels at the two ends of every model, between the waveform and the first or last conv block -- idv_stft_frames,
idv_stft_frames_kimage, idv_stft_frames_bwd, idv_istft_ola, idv_istft_ola_bwd, idv_make_dft, idv_mask_apply, idv_mask_apply_bwd,
idv_outtype_estimate, idv_datanorm, idv_datadenorm, idv_datanorm_bwd, idv_datadenorm_bwd, idv_planar_to_complex,
idv_complex_to_planar -- against the float64 reference of tests/signal_ref.py (itself checked on the CPU in
tests/test_signal_ref_host.py).  Every entry is called through the C ABI on buffers the test lays out itself (IDV_SLACK_FLOATS in
front and behind), so the test chooses pitches, Tp and alignment.  The case tables (signal_ref.py) are the smallest shapes that
reach each mechanism: two STFT geometries at the minimum length, at one 32-frame tile, one frame past it and the longest tail;
spectra at F in {1, 2, 5, 257}, T in {1, 2, 33}; B in {1, 3} and Tp in {T + 1, T + 3} everywhere; one case per element-wise entry
past the grid cap, where the stride loop runs.  Inputs are `exact` (integers in [-3, 3]) or `normal`.

Bounds, u = 2^-24.
  derived   idv_stft_frames, idv_planar_to_complex, idv_complex_to_planar: copies, every bit equal.
            idv_stft_frames_kimage: hi is x with its low 16 bits cleared, lo the bf16 nearest x - hi.  Integers in [-3, 3] have 2
            significant bits, so hi holds them and lo is 0; else |x - hi| < 2^-7 |x| and the rounding of lo leaves at most 2^-9 of
            that: |hi + lo - x| <= 2^-16 |x|.
            idv_istft_ola_bwd: one fp32 product, equal to fl32(dy * env_inv) with the device's own env_inv (and so within 2 u of
            the float64 value: the product and the rounding of the table).  idv_istft_ola, exact kind: the frame sum is an integer
            below 2^24, so the result equals fl32(sum * env_inv).  idv_stft_frames_bwd, exact kind: integer sums, equal.
            idv_make_dft: computed in double and rounded once, each entry within u |w| + 1e-12 of the float64 value.
            The build compiles with clang's default -ffp-contract=fast (a product may be fused into a following sum) and IEEE
            fp32 division (correctly rounded).  idv_datanorm is a difference, a sum std + 1e-6 and a quotient, nothing to fuse:
            3 u relative.  idv_datanorm_bwd: that sum and a quotient, 2 u.  idv_datadenorm_bwd: the sum of the two gradients and
            a product, 2 u.  idv_datadenorm is std * P + mean, which the compiler may fuse: it is judged as measured, and held
            to u (2 |std P| + |mean|) per element, which both forms meet.  Zeroed imaginary parts of bins 0 and F - 1 are +0.0.
            The mask gradient at M = 0 is fl(Gr xr + Gi xi), fl(Gi xr - Gr xi) of the summed gradient: 4 u (|Gr xr| + |Gi xi|).
  measured  idv_istft_ola and idv_stft_frames_bwd in the normal kind, the mask value and gradient, the three estimators,
            idv_datadenorm and the round trip: min(cap, 4 x the worst block measured on the MI355X with the cap as the bound),
            cap = TOL = 2e-5 for values and GTOL = 2e-4 for gradients (MEASURED below).  A block is one bin row
            of one utterance for spectra and one row for waveforms, judged by its relative L2 error and by its largest element
            error over its largest reference element; the worst block of every call is printed.  No element is excluded: the
            envelope stays above 1.25 and the estimator inputs cannot cancel (test_signal_ref_host.py).

Layout and reads, in every case.  Every output is pre-filled with a sentinel and, in a second call, with another: the written
region must come out with the same bits, which exposes an element neither call writes and a call that does not repeat.  Guard
columns tp == 0 and T < tp < Tp of every planar output are exactly +0.0; pitch columns [B Tp, Jp), planes behind the last one and
both slacks keep their sentinel; dx gets all B L elements, y exactly hop (T - 1) per row.  Inputs carry 7.0 in their guard and
pitch columns; a third call with NaN there, in the planes behind and in the slacks around flat inputs (every sample of a row is
read by some frame, test_signal_ref_host.py, so no sample can be poisoned) returns the bits of the first.

Corrections these tests led to.
  idv_mask_apply cleared only column tp == 0 of `pred`; with Tp > T + 1 the columns T < tp < Tp kept what the buffer held (the
      sentinel here, whatever torch.empty returned in ops.mask_apply).  It now clears both, as idv_mask_apply_bwd does.
      idv_stft_frames and idv_stft_frames_kimage left the same columns of the frames unwritten; they now write zeros.
  idv_datanorm, idv_datadenorm, their gradients and idv_outtype_estimate cleared their output with one memset over [2 F][Jp],
      pitch columns included; they now clear the guard columns alone.
  idv_mask_apply, idv_mask_apply_bwd, idv_planar_to_complex accepted Tp < T + 1, and with idv_istft_ola, the data_norm entries
      and idv_complex_to_planar Jp < B Tp; the two mask entries any JpX.  All are IDV_EINVAL now."""
import re

import pytest
import torch

import signal_ref as R

pytestmark = pytest.mark.gpu
TOL, GTOL = 2e-5, 2e-4       # the project's caps for forward values and for gradients
U = 2.0 ** -24
ONE = 1 + 1e-6               # room for the second-order terms of a derived bound
SENT = (-12345.0, 54321.0)
SENT16 = (0x5A5A, 0x3C3C)
EXTRA, BEHIND, PAD, FILL = 4, 8, 3, 7.0
NAN = float("nan")
# The worst block measured on the MI355X with the caps as bounds, per entry and kind: (relative L2, largest element error over
# largest reference element).  The asserted bound is min(cap, 4 x this).
MEASURED = {
    ("stft_frames_bwd", "normal"): (5.83e-08, 1.04e-07), ("istft_ola", "normal"): (6.75e-08, 1.35e-07),
    ("mask_apply", "exact"): (1.07e-07, 1.08e-07), ("mask_apply", "normal"): (2.02e-07, 2.09e-07),
    # the gradient's worst blocks are single bins (T = 1) with a large |M|, where (g' - g / |M|) (G . q) u and the part of
    # (g / |M|) conj(X) G along u cancel: of g / |M| ~ 0.24 each, g' = 1 - g^2 < 1e-3 is left
    ("mask_apply_bwd", "exact"): (3.77e-05, 3.77e-05), ("mask_apply_bwd", "normal"): (1.01e-05, 1.29e-05),
    ("mask_apply_bwd_dx", "exact"): (1.46e-07, 1.47e-07), ("mask_apply_bwd_dx", "normal"): (2.21e-07, 2.22e-07),
    ("estimate0", "exact"): (2.03e-07, 2.03e-07), ("estimate0", "normal"): (3.48e-07, 3.48e-07),
    ("estimate1", "exact"): (2.10e-07, 2.38e-07), ("estimate1", "normal"): (2.29e-07, 2.55e-07),
    ("estimate2", "exact"): (2.13e-07, 2.31e-07), ("estimate2", "normal"): (3.36e-07, 3.41e-07),
    ("datadenorm", "exact"): (0.0, 0.0), ("datadenorm", "normal"): (5.57e-08, 5.87e-08),       # exact: std 1, 2 or 4 -- no rounding
    ("round_trip", "stft"): (5.29e-07, 1.24e-06), ("round_trip", "mask"): (5.90e-07, 1.15e-06), ("round_trip", "istft"): (5.28e-07, 6.67e-07),
    ("round_trip", "istft_bwd"): (6.08e-07, 1.20e-06), ("round_trip", "stft_bwd"): (4.07e-07, 5.41e-07),
}
MISSED = []


def bound(entry, kind, cap, which):
    m = MEASURED.get((entry, kind))
    return cap if m is None else min(cap, 4 * m[which])


@pytest.fixture(autouse=True)
def no_missed_bound_left_over():
    MISSED.clear()


def judge(entry, kind, cap, what, got, want, dims):
    """Print the worst block of one call and hold it to the entry's bound.  A miss is noted and raised by settle() at the end of
    the test, so that the layout, repeatability and read checks behind it still run."""
    errs = R.worst_block(got, want, dims)
    bounds = [bound(entry, kind, cap, k) for k in range(2)]
    print("SIGNAL-MEASURE\t" + "\t".join([entry, kind] + [f"{e:.3e}" for e in errs]) + f"\t{what} (bounds {bounds})")
    if not all(e < b or e == 0 for e, b in zip(errs, bounds)):
        MISSED.append(f"{entry} {kind} {what}: {errs} against {bounds}")


def settle():
    assert not MISSED, "; ".join(MISSED)


@pytest.fixture(scope="module")
def ops(amd):
    with open(amd.ops.L.HEADER_PATH) as f:
        assert int(re.search(r"#define\s+IDV_SLACK_FLOATS\s+(\d+)", f.read()).group(1)) == amd.ops.SLACK
    return amd.ops


# ----------------------------------------------------------------------------- buffers
class Buf:
    """n floats with ops.SLACK floats in front and behind, `shift` floats off 16-byte alignment, filled with `fill`."""

    def __init__(self, ops, n, fill, shift=0, v=None):
        self.ops, self.n, self.off, self.fill = ops, n, ops.SLACK + shift, fill
        self.flat = torch.full((n + 2 * ops.SLACK + 4,), fill, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.body = self.flat[self.off:self.off + n]
        if v is not None:
            self.body[:] = v.reshape(-1).to(self.flat)

    def ptr(self, skip=0):
        return self.ops.L._P(self.flat.data_ptr() + 4 * (self.off + skip))

    def bits(self):
        return self.flat.view(torch.int32)

    def written(self):
        return self.body.view(torch.int32)

    def slacks_kept(self):
        return bool((self.flat[:self.off] == self.fill).all()) and bool((self.flat[self.off + self.n:] == self.fill).all())

    def check(self, what):
        assert self.slacks_kept(), f"{what}: written outside its {self.n} floats"

    def poison(self):
        self.flat[:self.off] = NAN
        self.flat[self.off + self.n:] = NAN


class Planar(Buf):
    """Planar rows [rows + behind][Jp], Jp = B Tp + PAD: v [rows, B, T] on the valid columns, `fill` everywhere else."""

    def __init__(self, ops, rows, B, T, Tp, fill, v=None, behind=EXTRA):
        self.rows, self.B, self.T, self.Tp, self.J, self.Jp = rows, B, T, Tp, B * Tp, B * Tp + PAD
        super().__init__(ops, (rows + behind) * self.Jp, fill)
        self.plane = self.body.view(rows + behind, self.Jp)
        if v is not None:
            R.place_planar(self.plane, v.cuda(), Tp)

    def valid(self):
        return R.read_planar(self.plane, self.rows, self.B, self.T, self.Tp)

    def spec(self):
        """[B, F, T, 2] of a spectrum's 2 F rows."""
        return R.rows_spec(self.valid())

    def written(self):
        return self.plane[:self.rows, :self.J].contiguous().view(torch.int32)

    def check(self, what):
        g = self.plane[:self.rows, :self.J][:, R.guard_mask(self.B, self.T, self.Tp, "cuda")]
        assert bool((g == 0).all()) and not bool(torch.signbit(g).any()), f"{what}: a guard column (tp == 0 or tp > T) is not +0.0"
        assert bool((self.plane[:self.rows, self.J:] == self.fill).all()), f"{what}: the pitch columns [B Tp, Jp) were written"
        assert bool((self.plane[self.rows:] == self.fill).all()), f"{what}: planes behind the last one were written"
        assert self.slacks_kept(), f"{what}: a slack was written"

    def poison(self):
        super().poison()
        self.plane[:self.rows, :self.J][:, R.guard_mask(self.B, self.T, self.Tp, "cuda")] = NAN
        self.plane[:self.rows, self.J:] = NAN
        self.plane[self.rows:] = NAN


class KImg:
    """The K-major split image of idv_stft_frames_kimage: KO octets x Jp columns x 8 bf16, a hi and a lo plane lo_off apart,
    64 halfwords of sentinel in front, between and behind."""

    def __init__(self, ops, win, B, T, Tp, fill):
        self.ops, self.win, self.B, self.T, self.Tp, self.J, self.Jp, self.fill = ops, win, B, T, Tp, B * Tp, B * Tp + PAD, fill
        self.KO = (win + 63) // 64 * 8
        n = self.KO * self.Jp * 8
        self.lo_off = n + 64
        self.flat = torch.full((64 + n + 64 + n + 64,), fill, dtype=torch.int16, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.hi, self.lo = (self.flat[o:o + n].view(self.KO, self.Jp, 8) for o in (64, 64 + self.lo_off))
        self.gaps = [self.flat[o:o + 64] for o in (0, 64 + n, 64 + self.lo_off + n)]

    def ptr(self):
        return self.ops.L._P(self.flat.data_ptr() + 2 * 64)

    def bits(self):
        return self.flat

    def written(self):
        return torch.stack((self.hi[:, :self.J], self.lo[:, :self.J]))

    def rows(self, plane):
        """-> (the 16-bit patterns, their values) as [8 KO, B, T]: sample k of frame (b, t)."""
        r = plane.permute(0, 2, 1).reshape(8 * self.KO, self.Jp)
        r = R.read_planar(r, 8 * self.KO, self.B, self.T, self.Tp)
        return r, (r.to(torch.int32) << 16).view(torch.float32)

    def check(self, what):
        g = R.guard_mask(self.B, self.T, self.Tp, "cuda")
        for p in (self.hi, self.lo):
            assert bool((p[:, :self.J][:, g] == 0).all()), f"{what}: a guard column's slot is not zero"
            assert bool((p[:, self.J:] == self.fill).all()), f"{what}: the pitch columns [B Tp, Jp) were written"
            assert bool((self.rows(p)[0][self.win:] == 0).all()), f"{what}: a sample at or past win is not zero"
        assert all(bool((t == self.fill).all()) for t in self.gaps), f"{what}: written outside the two planes"


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


READS = "guard columns, pitch columns, planes behind the last one or a slack of an input reach the result"


def same_f32(got, want):
    """Every bit equal (want: float64 holding fp32 values)."""
    return torch.equal(got.contiguous().view(torch.int32), want.float().contiguous().view(torch.int32))


def within(got, want, room):
    return bool(((got.double() - want).abs() <= room * ONE).all())


def seed_of(table, name, salt=0):
    return 1000 * salt + 10 * list(table).index(name)


_TABLES = {}


def tables(ops, geom, T):
    """The device's own idv_make_dft tables (w_fwd, w_inv, env_inv) of a geometry, as flat fp32 tensors."""
    if (geom, T) not in _TABLES:
        n_fft, win, hop = geom
        F, L = n_fft // 2 + 1, ops.L
        t = [torch.empty(n, device="cuda") for n in (2 * F * win, win * 2 * F, n_fft + hop * (T - 1))]
        L.call("idv_make_dft", L.i(n_fft), L.i(win), L.i(hop), L.i(T), L.p(t[0]), L.p(t[1]), L.p(t[2]), L.stream_ptr())
        torch.cuda.synchronize()
        _TABLES[geom, T] = t
    return _TABLES[geom, T]


def wave_case(name):
    c = R.WAVE_CASES[name]
    (n_fft, win, hop), B, Ln = c["geom"], c["B"], c["L"]
    T = R.n_frames(Ln, hop)
    return c["geom"], n_fft, win, hop, B, Ln, T, T + c["dTp"]


# ----------------------------------------------------------------------------- framing
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.WAVE_CASES))
def test_stft_frames_and_the_split_image(ops, name, kind):
    L = ops.L
    geom, n_fft, win, hop, B, Ln, T, Tp = wave_case(name)
    xv = R.gen(kind, (B, Ln), seed_of(R.WAVE_CASES, name)).cuda()
    x = Buf(ops, B * Ln, FILL, shift=B % 2, v=xv)
    want = R.frames(xv, *geom)
    geo = (x.ptr(), L.i(B), L.i(Ln), L.i(n_fft), L.i(win), L.i(hop), L.i(T))

    make = lambda k: [Planar(ops, win, B, T, Tp, SENT[k], behind=BEHIND)]
    launch = lambda o: L.call("idv_stft_frames", *geo, o[0].ptr(), L.i(Tp), L.i(o[0].Jp), L.stream_ptr())
    first = run(launch, make)
    assert same_f32(first[0].valid(), want), "idv_stft_frames: a frame sample differs from the signal's"

    make_k = lambda k: [KImg(ops, win, B, T, Tp, SENT16[k])]
    launch_k = lambda o: L.call("idv_stft_frames_kimage", *geo, o[0].ptr(), L.ll(o[0].lo_off), L.i(Tp), L.i(o[0].Jp), L.stream_ptr())
    img = run(launch_k, make_k)
    (_, hi), (lo_bits, lo) = img[0].rows(img[0].hi), img[0].rows(img[0].lo)
    if kind == "exact":
        assert same_f32(hi[:win], want) and bool((lo_bits == 0).all()), "idv_stft_frames_kimage: hi is not the integer, or lo is not 0"
    else:
        err = ((hi[:win].double() + lo[:win].double() - want).abs() / want.abs()).max()
        print(f"idv_stft_frames_kimage {name}: |hi + lo - x| / |x| {float(err):.3e} (bound {2.0 ** -16:.3e})")
        assert float(err) <= 2.0 ** -16
        assert torch.equal(hi[:win].view(torch.int32), first[0].valid().contiguous().view(torch.int32) & -65536)
    x.poison()
    rerun(launch, make, first, READS)
    rerun(launch_k, make_k, img, READS)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.WAVE_CASES))
def test_stft_frames_bwd(ops, name, kind):
    L = ops.L
    geom, n_fft, win, hop, B, Ln, T, Tp = wave_case(name)
    dv = R.gen(kind, (win, B, T), seed_of(R.WAVE_CASES, name, 1)).cuda()
    dfr = Planar(ops, win, B, T, Tp, FILL, dv)
    want = R.frames_adj(dv, Ln, *geom)
    make = lambda k: [Buf(ops, B * Ln, SENT[k], shift=B % 2)]
    launch = lambda o: L.call("idv_stft_frames_bwd", dfr.ptr(), L.i(B), L.i(Ln), L.i(n_fft), L.i(win), L.i(hop), L.i(T), L.i(Tp),
                              L.i(dfr.Jp), o[0].ptr(), L.stream_ptr())
    first = run(launch, make)                                      # all B L elements written: the two sentinels agree nowhere
    got = first[0].body.view(B, Ln)
    if kind == "exact":
        assert torch.equal(got.double(), want), "idv_stft_frames_bwd: an integer sum differs"
    else:
        judge("stft_frames_bwd", kind, GTOL, name, got, want, R.WAVE_BLOCK)
    dfr.poison()
    rerun(launch, make, first, READS)
    settle()


# ----------------------------------------------------------------------------- overlap-add
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.WAVE_CASES))
def test_istft_ola_and_its_gradient(ops, name, kind):
    L = ops.L
    geom, n_fft, win, hop, B, Ln, T, Tp = wave_case(name)
    half, Lout = n_fft // 2, hop * (T - 1)
    env = tables(ops, geom, T)[2]
    env64 = R.dft_tables(n_fft, win, hop, T)[2].cuda()
    fv = R.gen(kind, (win, B, T), seed_of(R.WAVE_CASES, name, 2)).cuda()
    fr = Planar(ops, win, B, T, Tp, FILL, fv)
    geo = (L.i(B), L.i(n_fft), L.i(win), L.i(hop), L.i(T), L.i(Tp), L.i(fr.Jp))
    make = lambda k: [Buf(ops, B * Lout, SENT[k], shift=B % 2)]
    launch = lambda o: L.call("idv_istft_ola", fr.ptr(), L.p(env), *geo, o[0].ptr(), L.stream_ptr())
    first = run(launch, make)                                      # exactly hop (T - 1) samples per row: all written, no slack touched
    got = first[0].body.view(B, Lout)
    if kind == "exact":
        total = R.ola_sum(fv, *geom)
        assert float(total.abs().max()) < 2 ** 24
        assert torch.equal(got, total.float() * env[half:half + Lout]), "idv_istft_ola: not fl32(the integer sum * env_inv)"
    else:
        judge("istft_ola", kind, TOL, name, got, R.ola(fv, env64, *geom), R.WAVE_BLOCK)

    dyv = R.gen(kind, (B, Lout), seed_of(R.WAVE_CASES, name, 3)).cuda()
    dy = Buf(ops, B * Lout, FILL, shift=1 - B % 2, v=dyv)
    make_b = lambda k: [Planar(ops, win, B, T, Tp, SENT[k], behind=BEHIND)]
    launch_b = lambda o: L.call("idv_istft_ola_bwd", dy.ptr(), L.p(env), *geo, o[0].ptr(), L.stream_ptr())
    grad = run(launch_b, make_b)
    g32, e32 = R.ola_adj_parts(dyv, env, T, *geom)
    assert torch.equal(grad[0].valid(), g32 * e32), "idv_istft_ola_bwd: not fl32(dy * env_inv), or not 0 outside the kept range"
    want = R.ola_adj(dyv, env64, T, *geom)
    assert within(grad[0].valid(), want, 2 * U * want.abs()), "idv_istft_ola_bwd: more than 2 u from the float64 value"
    fr.poison()
    dy.poison()
    rerun(launch, make, first, READS)
    rerun(launch_b, make_b, grad, READS)
    settle()


@pytest.mark.parametrize("T", R.ENV_T)
@pytest.mark.parametrize("gname", list(R.GEOMS))
def test_make_dft(ops, gname, T):
    L = ops.L
    n_fft, win, hop = R.GEOMS[gname]
    F = n_fft // 2 + 1
    sizes = (2 * F * win, win * 2 * F, n_fft + hop * (T - 1))
    make = lambda k: [Buf(ops, n, SENT[k], shift=s) for n, s in zip(sizes, (0, 1, 2))]
    launch = lambda o: L.call("idv_make_dft", L.i(n_fft), L.i(win), L.i(hop), L.i(T), o[0].ptr(), o[1].ptr(), o[2].ptr(), L.stream_ptr())
    first = run(launch, make)
    for what, got, want in zip(("w_fwd", "w_inv", "env_inv"), first, R.dft_tables(n_fft, win, hop, T)):
        want = want.reshape(-1).cuda()
        err = (got.body.double() - want).abs()
        room = U * want.abs() + 1e-12
        print(f"idv_make_dft {gname} T {T} {what}: largest error over its bound {float((err / room).max()):.3f}")
        assert bool((err <= room).all()), f"{what}: an entry is more than u |w| + 1e-12 from the float64 table"
    assert bool((first[2].body[n_fft // 2:n_fft // 2 + hop * (T - 1)] > 0).all())


# ----------------------------------------------------------------------------- spectra
def spec_case(name):
    c = R.SPEC_CASES[name]
    return c["F"], c["B"], c["T"], c["T"] + c["dTp"], (("normal",) if name == "cap" else R.KINDS)


SPEC = [(n, k) for n in R.SPEC_CASES for k in spec_case(n)[4]]


def spec_in(ops, v, Tp):
    """A spectrum [B, F, T, 2] as a planar input: 7.0 in its guard and pitch columns and in EXTRA planes behind."""
    B, F, T, _ = v.shape
    return Planar(ops, 2 * F, B, T, Tp, FILL, R.spec_rows(v))


@pytest.mark.parametrize("name,kind", SPEC)
def test_mask_and_its_gradient(ops, name, kind):
    L = ops.L
    F, B, T, Tp, _ = spec_case(name)
    seed = seed_of(R.SPEC_CASES, name, 4)
    Mv = R.gen_mask(kind, B, F, T, seed).cuda()
    zero = (Mv == 0).all(dim=-1)
    Gv, Gcv = R.gen(kind, (B, F, T, 2), seed + 1).cuda(), R.gen(kind, (B, F, T, 2), seed + 2).cuda()
    M, dpred, dpred_c = spec_in(ops, Mv, Tp), spec_in(ops, Gv, Tp), Buf(ops, B * F * T * 2, FILL, shift=1, v=Gcv)
    for x_div in ([1] if name == "cap" else R.x_divs(B)):
        Xv = R.gen(kind, (B // x_div, F, T, 2), seed + 3 + x_div).cuda()
        X = spec_in(ops, Xv, Tp)
        geo = (L.i(F), L.i(B), L.i(T), L.i(Tp), L.i(M.Jp))
        head = (M.ptr(), X.ptr(), L.i(x_div), L.i(X.Jp))
        what = f"{name} x_div {x_div}"

        make = lambda k: [Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND), Buf(ops, B * F * T * 2, SENT[k], shift=1)]
        launch = lambda o: L.call("idv_mask_apply", *head, o[0].ptr(), o[1].ptr(), *geo, L.stream_ptr())
        first = run(launch, make)
        got, want = first[0].spec(), R.mask(Mv, Xv, x_div)
        judge("mask_apply", kind, TOL, what, got, want, R.SPEC_BLOCK)
        assert bool((got[zero] == 0).all()), "idv_mask_apply: the prediction at M = 0 is not 0"
        assert torch.equal(first[1].body.view(B, F, T, 2), got), "idv_mask_apply: pred_c differs from pred"
        alone = run(lambda o: L.call("idv_mask_apply", *head, o[0].ptr(), L.p(None), *geo, L.stream_ptr()), lambda k: make(k)[:1])
        assert torch.equal(alone[0].bits(), first[0].bits()), "idv_mask_apply: pred depends on pred_c"

        grads = {}
        for use_p, use_c in ((True, True),) if name == "cap" else ((True, True), (True, False), (False, True)):
            def make_b(k):
                o = [Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND)]
                return o + ([Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND)] if x_div == 1 else [])

            def launch_b(o, use_p=use_p, use_c=use_c):
                L.call("idv_mask_apply_bwd", *head, dpred.ptr() if use_p else L.p(None), dpred_c.ptr() if use_c else L.p(None), *geo,
                       o[0].ptr(), o[1].ptr() if x_div == 1 else L.p(None), L.stream_ptr())

            g = run(launch_b, make_b)
            grads[use_p, use_c] = (launch_b, make_b, g)
            Gsum = (Gv.double() if use_p else 0) + (Gcv.double() if use_c else 0)
            dM, dX = R.mask_bwd(Mv, Xv, x_div, Gsum)
            gotM = g[0].spec()
            judge("mask_apply_bwd", kind, GTOL, f"{what} dpred {use_p} dpred_c {use_c}", gotM, dM, R.SPEC_BLOCK)
            Gz, xz = Gsum[zero], R.spectrum_rows(Xv.double(), B, x_div)[zero]
            cross = lambda a, b: (Gz[:, a] * xz[:, 0]).abs() + (Gz[:, b] * xz[:, 1]).abs()
            room = 4 * U * torch.stack((cross(0, 1), cross(1, 0)), dim=-1)         # (Gr xr + Gi xi, Gi xr - Gr xi)
            assert within(gotM[zero], dM[zero], room), "idv_mask_apply_bwd: the gradient at M = 0 is not the limit conj(X) G"
            if x_div == 1:
                gotX = g[1].spec()
                judge("mask_apply_bwd_dx", kind, GTOL, f"{what} dpred {use_p} dpred_c {use_c}", gotX, dX, R.SPEC_BLOCK)
                assert bool((gotX[zero] == 0).all()), "idv_mask_apply_bwd: dX at M = 0 is not 0"
        for b in (M, X, dpred, dpred_c):
            b.poison()
        rerun(launch, make, first, READS)
        for launch_b, make_b, g in grads.values():
            rerun(launch_b, make_b, g, READS)
        M, dpred, dpred_c = spec_in(ops, Mv, Tp), spec_in(ops, Gv, Tp), Buf(ops, B * F * T * 2, FILL, shift=1, v=Gcv)
    settle()


@pytest.mark.parametrize("name,kind", SPEC)
def test_estimators(ops, name, kind):
    L = ops.L
    F, B, T, Tp, _ = spec_case(name)
    for ns in ((1,) if name == "cap" else R.NS):
        sv, nv, Xv = (t.cuda() for t in R.gen_estimator(kind, B, ns, F, T, 700 + ns))          # the draws the CPU test checks
        speech, noise = Buf(ops, sv.numel(), FILL, v=sv), Buf(ops, nv.numel(), FILL, shift=1, v=nv)
        flat, planar = Buf(ops, Xv.numel(), FILL, shift=2, v=Xv), spec_in(ops, Xv, T + 2)
        layouts = {"contiguous": (flat.ptr(), (F * T * 2, T * 2, 2, 1)),
                   "planar view": (planar.ptr(1), (planar.Tp, planar.Jp, 1, F * planar.Jp))}        # (sb, sf, st, sr) from column 1
        runs = []
        for mode in range(3):
            want = R.estimate(mode, sv, nv, Xv, ns)
            for lname, (xptr, strides) in layouts.items():
                make = lambda k: [Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND), Buf(ops, B * F * T * 2, SENT[k], shift=1)]

                def launch(o, mode=mode, xptr=xptr, strides=strides, c=True):
                    L.call("idv_outtype_estimate", speech.ptr(), noise.ptr(), xptr, *(L.ll(s) for s in strides), L.i(mode), L.i(ns), L.i(B),
                           L.i(F), L.i(T), L.i(Tp), L.i(o[0].Jp), o[0].ptr(), o[1].ptr() if c else L.p(None), L.stream_ptr())

                first = run(launch, make)
                runs.append((launch, make, first))
                got = first[0].spec()
                judge(f"estimate{mode}", kind, TOL, f"{name} ns {ns} X {lname}", got, want, R.SPEC_BLOCK)
                assert torch.equal(first[1].body.view(B, F, T, 2), got), "idv_outtype_estimate: out_c differs from out"
            alone = run(lambda o: launch(o, c=False), lambda k: make(k)[:1])
            assert torch.equal(alone[0].bits(), first[0].bits()), "idv_outtype_estimate: out depends on out_c"
        assert torch.equal(runs[0][2][0].bits(), runs[1][2][0].bits()), "the two layouts of X give different bits"
        for b in (speech, noise, flat, planar):
            b.poison()
        for launch, make, first in runs:
            rerun(launch, make, first, READS)
    settle()


@pytest.mark.parametrize("name,kind", SPEC)
def test_data_norm_and_its_gradients(ops, name, kind):
    L = ops.L
    F, B, T, Tp, _ = spec_case(name)
    seed = seed_of(R.SPEC_CASES, name, 5)
    mean, std = (t.cuda() for t in R.gen_stats(kind, F, seed))
    Xv, Gv, Gcv = (R.gen(kind, (B, F, T, 2), seed + k).cuda() for k in (1, 2, 3))
    X, G, Gc = spec_in(ops, Xv, Tp), spec_in(ops, Gv, Tp), Buf(ops, Gcv.numel(), FILL, shift=1, v=Gcv)
    geo = (L.i(F), L.i(B), L.i(T), L.i(Tp), L.i(X.Jp))
    edges = lambda v: torch.stack((v[:, 0, :, 1], v[:, F - 1, :, 1]))           # the imaginary parts of the first and the last bin
    out1 = lambda k: [Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND)]
    out2 = lambda k: out1(k) + [Buf(ops, B * F * T * 2, SENT[k], shift=1)]
    runs = []

    def held(entry, launch, make, want, room):
        first = run(launch, make)
        runs.append((launch, make, first))
        got = first[0].spec()
        err = (got.double() - want).abs()
        ratio = float((err / room.clamp_min(1e-300)).max())
        print(f"{entry} {name} {kind}: largest error over its bound {ratio:.3f}")
        assert within(got, want, room), f"{entry}: outside its derived bound"
        return first, got

    want = R.datanorm(Xv, mean, std)
    _, got = held("idv_datanorm", lambda o: L.call("idv_datanorm", X.ptr(), L.p(mean), L.p(std), *geo, o[0].ptr(), L.stream_ptr()), out1,
                  want, 3 * U * want.abs())
    z = edges(got)
    assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "idv_datanorm: the imaginary part of bin 0 or F - 1 is not +0.0"
    want = R.datanorm_bwd(Gv, std)
    _, got = held("idv_datanorm_bwd", lambda o: L.call("idv_datanorm_bwd", G.ptr(), L.p(std), *geo, o[0].ptr(), L.stream_ptr()), out1,
                  want, 2 * U * want.abs())
    z = edges(got)
    assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "idv_datanorm_bwd: bin 0 or F - 1 sends an imaginary gradient"
    want = R.datadenorm(Xv, mean, std)
    sP = (std.double()[None, :, None, :] * Xv.double()).abs()
    first, got = held("idv_datadenorm", lambda o: L.call("idv_datadenorm", X.ptr(), L.p(mean), L.p(std), *geo, o[0].ptr(), o[1].ptr(),
                                                         L.stream_ptr()), out2, want, U * (2 * sP + mean.double().abs()[None, :, None, :]))
    judge("datadenorm", kind, TOL, name, got, want, R.SPEC_BLOCK)
    assert torch.equal(first[1].body.view(B, F, T, 2), got), "idv_datadenorm: out_c differs from out"
    for use_p, use_c in ((True, True), (True, False), (False, True)):
        want = R.datadenorm_bwd(Gv if use_p else None, Gcv if use_c else None, std)
        held(f"idv_datadenorm_bwd dout {use_p} dout_c {use_c}",
             lambda o, p=use_p, c=use_c: L.call("idv_datadenorm_bwd", G.ptr() if p else L.p(None), Gc.ptr() if c else L.p(None), L.p(std), *geo,
                                                o[0].ptr(), L.stream_ptr()), out1, want, 2 * U * want.abs())
    for b in (X, G, Gc):
        b.poison()
    for launch, make, first in runs:
        rerun(launch, make, first, READS)
    settle()


@pytest.mark.parametrize("name,kind", SPEC)
def test_converters(ops, name, kind):
    L = ops.L
    F, B, T, Tp, _ = spec_case(name)
    Xv = R.gen(kind, (B, F, T, 2), seed_of(R.SPEC_CASES, name, 6)).cuda()
    X, Xc = spec_in(ops, Xv, Tp), Buf(ops, Xv.numel(), FILL, shift=1, v=Xv)
    geo = (L.i(F), L.i(B), L.i(T), L.i(Tp), L.i(X.Jp))
    make = lambda k: [Buf(ops, Xv.numel(), SENT[k], shift=1)]
    launch = lambda o: L.call("idv_planar_to_complex", X.ptr(), o[0].ptr(), *geo, L.stream_ptr())
    first = run(launch, make)
    assert same_f32(first[0].body.view(B, F, T, 2), Xv), "idv_planar_to_complex: a bit differs"
    make_b = lambda k: [Planar(ops, 2 * F, B, T, Tp, SENT[k], behind=BEHIND)]
    launch_b = lambda o: L.call("idv_complex_to_planar", Xc.ptr(), o[0].ptr(), *geo, L.stream_ptr())
    back = run(launch_b, make_b)
    assert same_f32(back[0].spec(), Xv), "idv_complex_to_planar: a bit differs"
    X.poison()
    Xc.poison()
    rerun(launch, make, first, READS)
    rerun(launch_b, make_b, back, READS)


# ----------------------------------------------------------------------------- refusals
def test_invalid_arguments_write_nothing(ops):
    """Every refusal is IDV_EINVAL and comes before any launch: all destinations keep their sentinel.  Every buffer has the size
    of the valid call (F = 5, B = 3, T = 9, Tp = 12; the small STFT geometry at L = 395), so even a call that were not refused
    would stay inside it."""
    L = ops.L
    F, B, T, Tp = 5, 3, 9, 12
    n_fft, win, hop = R.GEOMS["small"]
    Ln = 395
    Tw = R.n_frames(Ln, hop)
    Tpw = Tw + 3
    src = Planar(ops, 2 * F, B, T, Tp, 1.0)
    cpx = Buf(ops, 5 * B * F * T * 2, 1.0)
    wav, frs, env = Buf(ops, B * Ln, 1.0), Planar(ops, win, B, Tw, Tpw, 1.0), torch.ones(n_fft + hop * Tw, device="cuda")
    dst, dst2, dstw = Planar(ops, 2 * F, B, T, Tp, SENT[0]), Buf(ops, B * F * T * 2, SENT[0]), Planar(ops, win, B, Tw, Tpw, SENT[0])
    dsty, img = Buf(ops, B * Ln, SENT[0]), KImg(ops, win, B, Tw, Tpw, SENT16[0])
    stat = torch.ones(F, 2, device="cuda")
    s = L.stream_ptr()

    def refused(entry, good, bad):
        for kw in bad:
            a = dict(good, **kw)
            with pytest.raises(L.IdvError, match=r"status -1 "):
                L.call(entry, *[L.p(None) if v is None else (L.i(v) if isinstance(v, int) else v) for v in a.values()], s)

    geo = dict(F=F, B=B, T=T, Tp=Tp, Jp=src.Jp)
    bad = [dict(Tp=T), dict(Jp=B * Tp - 1)]
    mk = dict(mask=src.ptr(), X=src.ptr(), x_div=1, JpX=src.Jp, pred=dst.ptr(), pred_c=dst2.ptr(), **geo)
    refused("idv_mask_apply", mk, bad + [dict(x_div=0), dict(JpX=B * Tp - 1)])
    mb = dict(mask=src.ptr(), X=src.ptr(), x_div=1, JpX=src.Jp, dpred=src.ptr(), dpred_c=cpx.ptr(), **geo, dmask=dst.ptr(), dX=dst.ptr())
    refused("idv_mask_apply_bwd", mb, bad + [dict(x_div=0), dict(x_div=3), dict(JpX=B * Tp - 1), dict(dpred=None, dpred_c=None)])
    est = dict(speech=cpx.ptr(), noise=cpx.ptr(), X=cpx.ptr(), sb=L.ll(F * T * 2), sf=L.ll(T * 2), st=L.ll(2), sr=L.ll(1), mode=1, ns=2, B=B,
               F=F, T=T, Tp=Tp, Jp=src.Jp, out=dst.ptr(), out_c=dst2.ptr())
    refused("idv_outtype_estimate", est, bad + [dict(mode=-1), dict(mode=3), dict(ns=0)])
    refused("idv_datanorm", dict(X=src.ptr(), mean=L.p(stat), stdv=L.p(stat), **geo, out=dst.ptr()), bad)
    refused("idv_datadenorm", dict(P=src.ptr(), mean=L.p(stat), stdv=L.p(stat), **geo, out=dst.ptr(), out_c=dst2.ptr()), bad)
    refused("idv_datanorm_bwd", dict(dout=src.ptr(), stdv=L.p(stat), **geo, dX=dst.ptr()), bad)
    refused("idv_datadenorm_bwd", dict(dout=src.ptr(), dout_c=cpx.ptr(), stdv=L.p(stat), **geo, dP=dst.ptr()), bad + [dict(dout=None, dout_c=None)])
    refused("idv_planar_to_complex", dict(act=src.ptr(), out_c=dst2.ptr(), **geo), bad)
    refused("idv_complex_to_planar", dict(in_c=cpx.ptr(), act=dst.ptr(), **geo), bad)
    fr = dict(x=wav.ptr(), B=B, L=Ln, n_fft=n_fft, win=win, hop=hop, T=Tw)
    badw = [dict(Tp=Tw), dict(Jp=B * Tpw - 1)]
    badl = [dict(L=n_fft // 2, T=R.n_frames(n_fft // 2, hop)), dict(T=Tw - 1), dict(T=Tw + 1)]
    refused("idv_stft_frames", dict(fr, frames=dstw.ptr(), Tp=Tpw, Jp=dstw.Jp), badw + badl)
    refused("idv_stft_frames_kimage", dict(fr, img=img.ptr(), lo_off=L.ll(img.lo_off), Tp=Tpw, Jp=img.Jp), badw + badl)
    refused("idv_stft_frames_bwd", dict(dframes=frs.ptr(), B=B, L=Ln, n_fft=n_fft, win=win, hop=hop, T=Tw, Tp=Tpw, Jp=frs.Jp, dx=dsty.ptr()),
            badw + badl)
    ola = dict(frames=frs.ptr(), env_inv=L.p(env), B=B, n_fft=n_fft, win=win, hop=hop, T=Tw, Tp=Tpw, Jp=frs.Jp)
    refused("idv_istft_ola", dict(ola, y=dsty.ptr()), badw + [dict(T=1)])
    refused("idv_istft_ola_bwd", dict(ola, frames=wav.ptr(), dframes=dstw.ptr()), badw + [dict(T=1)])
    torch.cuda.synchronize()
    for b in (dst, dst2, dstw, dsty):
        assert bool((b.flat == SENT[0]).all()), "a refused call wrote"
    assert bool((img.flat == SENT16[0]).all()), "a refused call wrote"


# ----------------------------------------------------------------------------- the public wrappers
def test_round_trip_through_the_wrappers(ops):
    """ops.stft -> ops.mask_apply -> ops.istft and ops.istft_bwd / ops.stft_bwd at (512, 400, 100), L = 3299, B = 3, Tp = T + 3,
    against the float64 chain.  This ties the direct calls above to what the models run: Planar.empty destinations (uninitialised
    memory) and the precision mode the package is in."""
    n_fft, win, hop = R.ROUND_TRIP["geom"]
    B, Ln = R.ROUND_TRIP["B"], R.ROUND_TRIP["L"]
    T, F = R.n_frames(Ln, hop), n_fft // 2 + 1
    Tp = T + R.ROUND_TRIP["dTp"]
    geom = (n_fft, win, hop)
    guard = R.guard_mask(B, T, Tp, "cuda")

    def guards_zero(pl, what):
        g = pl.data.view(-1, pl.Jp)[:, :B * Tp][:, guard]
        assert bool((g == 0).all()) and not bool(torch.signbit(g).any()), f"{what}: a guard column is not +0.0"

    junk = [ops.Planar.empty(1, F, B, T, Tp, "cuda") for _ in range(4)]       # what Planar.empty hands out next is not zero
    for j in junk:
        j.buf.fill_(SENT[0])
    del junk
    xv = R.gen("normal", (B, Ln), 1).cuda()
    Mv = R.gen_mask("normal", B, F, T, 2).cuda()
    plan = ops.DftPlan(n_fft, win, hop, T, "cuda")
    X = ops.stft(xv, plan, Tp=Tp)
    assert (X.Tp, X.T, X.B, X.F) == (Tp, T, B, F)
    guards_zero(X, "ops.stft")
    X64 = R.stft(xv, *geom)
    judge("round_trip", "stft", TOL, "ops.stft", X.tensor4(), X64, R.SPEC_BLOCK)
    M = ops.Planar.from_tensor5(Mv.unsqueeze(1), Tp=Tp)
    pred, pc = ops.mask_apply(M, X)
    guards_zero(pred, "ops.mask_apply")
    P64 = R.mask(Mv, X64)
    judge("round_trip", "mask", TOL, "ops.mask_apply", pred.tensor4(), P64, R.SPEC_BLOCK)
    assert torch.equal(torch.view_as_real(pc), pred.tensor4())
    y = ops.istft(pred, plan)
    assert tuple(y.shape) == (B, hop * (T - 1))
    judge("round_trip", "istft", TOL, "ops.istft", y, R.istft(P64, *geom), R.WAVE_BLOCK)
    dyv = R.gen("normal", (B, hop * (T - 1)), 3).cuda()
    w_fwd, w_inv, env_inv = (t.cuda() for t in R.dft_tables(n_fft, win, hop, T))
    dspec = ops.istft_bwd(dyv, pred, plan)
    guards_zero(dspec, "ops.istft_bwd")
    want = R.rows_spec(torch.tensordot(w_inv.t(), R.ola_adj(dyv, env_inv, T, *geom), dims=([1], [0])))
    judge("round_trip", "istft_bwd", GTOL, "ops.istft_bwd", dspec.tensor4(), want, R.SPEC_BLOCK)
    Gv = R.gen("normal", (B, F, T, 2), 4).cuda()
    dx = ops.stft_bwd(ops.Planar.from_tensor5(Gv.unsqueeze(1), Tp=Tp), plan, Ln)
    assert tuple(dx.shape) == (B, Ln)
    want = R.frames_adj(torch.tensordot(w_fwd.t(), R.spec_rows(Gv.double()), dims=([1], [0])), Ln, *geom)
    judge("round_trip", "stft_bwd", GTOL, "ops.stft_bwd", dx, want, R.WAVE_BLOCK)
    settle()
