"""The forward point-wise GEMM family -- idv_pw_gemm (csrc/cgemm.hip) and the bf16x3 entries idv_pw_bf16x3, idv_pw_bf16x3_rows,
idv_lstm_proj_bf16x3, idv_lstm_proj1_bf16x3 (csrc/pw_bf16.hip) -- against the float64 reference of tests/pw_ref.py (itself checked
on the CPU in tests/test_pw_ref_host.py).  Every entry is called through the C ABI on buffers the test lays out itself
(IDV_SLACK_FLOATS in front and behind, ops.KImage for the images), so the test and not ops.PRECISION or Planar chooses pitch,
alignment and kernel form.  Every case runs twice:

  exact   W, bias, x integers in [-3, 3], slope 0.25.  Every product and partial sum is an integer (or a multiple of 1/4) below
          2^24 in any summation order, and the integers are exact in a bf16 `hi` with `lo` = 0: the result must EQUAL the
          reference, for the fp32 and the bf16x3 entries alike.  No tolerance: a wrong index, mask, tile edge, permutation or
          store address changes an integer.
  normal  standard-normal x, 0.1 * standard-normal W, standard-normal bias, slope 0.25; relative L2 error per 32-row tile over
          all valid columns and per utterance over all rows.  fp32 entries against float64: TOL = 2e-5 (expected size
          sqrt(K) * 2^-24).  bf16x3 entries (a) against pw_ref.split_model, the same operation in exact arithmetic, so that only
          the fp32 accumulation remains: MODEL_TOL, per entry four times the worst block measured on the MI355X (2.28e-7 for the
          two generic entries, 8.99e-8 and 5.83e-8 for the two projections), far below the 2e-5 cap -- this is
          the comparison that notices a wrongly rounded `lo` or a weakened cross term (tests/test_pw_ref_host.py shows that
          either moves the model by more than these bounds); (b) against float64 over the whole tensor: TOL.  The worst block of
          every call is printed.

In every case: guard columns of the planar store are exactly 0.0; the pitch columns [J, Jp), 32 planes behind row M and both slacks
keep a pre-filled sentinel; the row-major store keeps it in the columns [M, ldo), in the rows from T * B on and in the slacks; NaN in
the pitch columns of every input plane and in 8 extra planes behind plane K changes not one output bit (NaN, not 1e30: the
weights of padded k are zero and 0 * 1e30 would hide a read); a second call returns the same bits.  The last test of the file
asserts that the forms the library's queries reported over all cases are all forms there are, so it needs the whole file."""
import re

import pytest
import torch

import pw_ref as R

pytestmark = pytest.mark.gpu
TOL = 2e-5                   # the project's bound for forward ops
# bf16x3 against the exact-arithmetic model: min(2e-5, 4 x the worst block measured with the bound at 2e-5), per entry
MODEL_TOL = {"pw": 4 * 2.28e-7, "proj": 4 * 8.99e-8, "proj1": 4 * 5.83e-8}
SENTINEL, EXTRA, BEHIND = -12345.0, 8, 32
KINDS = ["exact", "normal"]
SEEN_GEMM, SEEN_BF16 = set(), set()
CACHE = {}


@pytest.fixture(scope="module")
def ops(amd):
    with open(amd.ops.L.HEADER_PATH) as f:
        assert int(re.search(r"#define\s+IDV_SLACK_FLOATS\s+(\d+)", f.read()).group(1)) == amd.ops.SLACK
    return amd.ops


def draw(kind, shape, g, scale=1.0):
    if kind == "exact":
        return torch.randint(-3, 4, shape, generator=g, device="cuda").float()
    return scale * torch.randn(shape, generator=g, device="cuda")


def ceil4(n):
    return (n + 3) // 4 * 4


class Buf:
    """rows x pitch floats with ops.SLACK floats in front and behind, `shift` floats off 16-byte alignment, filled with `fill`."""

    def __init__(self, ops, rows, pitch, fill, shift=0):
        self.ops, self.n, self.off = ops, rows * pitch, ops.SLACK + shift
        self.flat = torch.full((self.n + 2 * ops.SLACK + 4,), fill, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.body = self.flat[self.off:self.off + self.n].view(rows, pitch)

    @property
    def addr(self):
        return self.flat.data_ptr() + 4 * self.off

    def ptr(self):
        return self.ops.L._P(self.addr)

    def slack_kept(self, fill):
        return bool((self.flat[:self.off] == fill).all()) and bool((self.flat[self.off + self.n:] == fill).all())


def input_planes(ops, v, Tp, Jp, shift=0):
    """v [planes, B, T] -> zeroed planar Buf of planes + EXTRA rows with the values at their columns."""
    buf = Buf(ops, v.shape[0] + EXTRA, Jp, 0.0, shift)
    R.place_planar(buf.body, v, Tp)
    return buf


def poison(buf, planes, J):
    buf.body[:planes, J:] = float("nan")
    buf.body[planes:] = float("nan")


def check_planar(out, M, B, T, Tp, J):
    body = out.body
    guard = R.guard_mask(B, T, Tp, body.device)
    zeros = body[:M, :J][:, guard]
    assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any()), "a guard column is not exactly 0.0"
    assert bool((body[:M, J:] == SENTINEL).all()), "the pitch columns [J, Jp) were written"
    assert bool((body[M:] == SENTINEL).all()), "planes behind row M were written"
    assert out.slack_kept(SENTINEL), "the slack in front of or behind the output was written"
    return R.read_planar(body, M, B, T, Tp)


def check_rows(out, M, B, T, ldo, parts=1):
    body = out.body
    assert bool((body[:parts * T * B, M:] == SENTINEL).all()), "the columns [M, ldo) were written"
    assert bool((body[parts * T * B:] == SENTINEL).all()), "rows at or behind T * B were written"
    assert out.slack_kept(SENTINEL), "the slack in front of or behind the output was written"
    return [R.read_rows(body[p * T * B:(p + 1) * T * B], M, B, T, ldo) for p in range(parts)]


def compare(what, kind, got, want, tol, whole=None):
    """got [M, B, T] against want (float64).  whole: a second reference held over the whole tensor to TOL."""
    if kind == "exact":
        assert float(want.abs().max()) < 2 ** 24
        bad = (got.double() != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {got.numel()} entries differ, first at (m, b, t) = {bad[0].tolist()}: " \
                                 f"{float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}"
        return
    tile, utt = R.block_errors(got, want)
    line = f"{what} normal: worst 32-row tile {tile:.2e}, worst utterance {utt:.2e} (bound {tol:.1e})"
    if whole is not None:
        err = R.rel_l2(got, whole)
        line += f"; whole tensor against float64 {err:.2e} (bound {TOL:.0e})"
    print(line)
    assert tile < tol and utt < tol, line
    if whole is not None:
        assert err < TOL, line


# ----------------------------------------------------------------------------- idv_pw_gemm
def pack_lstm_ih(ops, H, K, ws):
    """idv_pack_lstm_ih of (w_re, w_im, b_ih_re, b_hh_re, b_ih_im, b_hh_im) -> (fp32 fragments, bias [8H padded], gate order)."""
    L = ops.L
    w_re, w_im, b_ih_re, b_hh_re, b_ih_im, b_hh_im = ws
    mt, ks = ops.mtiles_alloc(8 * H), (K + 7) // 8 * 4
    wfrag, bout = torch.empty(mt * ks * 64, device="cuda"), torch.empty(mt * 32, device="cuda")
    L.call("idv_pack_lstm_ih", L.p(w_re), L.p(b_ih_re), L.p(b_hh_re), L.p(w_im), L.p(b_ih_im), L.p(b_hh_im), L.i(H), L.i(K), L.p(wfrag),
           L.p(bout), L.stream_ptr())
    return wfrag, bout


def draw_lstm(kind, H, K, g):
    return tuple(draw(kind, (4 * H, K), g, 0.1) for _ in range(2)) + tuple(draw(kind, (4 * H,), g) for _ in range(4))


def gemm_operands(ops, name, kind):
    """Operands and float64 reference of a case, once for its store and staging variants."""
    key = ("gemm", name, kind)
    if key not in CACHE:
        M, K, B, T, Tp, use_slope, _, H = R.GEMM_CASES[name]
        g = torch.Generator(device="cuda").manual_seed(1000 + list(R.GEMM_CASES).index(name))
        xv = draw(kind, (K, B, T), g)
        if H:
            ws = draw_lstm(kind, H, K, g)
            wfrag, bout = pack_lstm_ih(ops, H, K, ws)
            w, bias = R.lstm_stack(ws[0], ws[1], *ws[2:], H)
        else:
            w, bias = draw(kind, (M, K), g, 0.1), draw(kind, (M,), g)
            wfrag, bout = ops.pack_pw(w, bias)
        slope = torch.tensor([0.25], device="cuda") if use_slope else None
        CACHE[key] = (xv, wfrag, bout, slope, R.pw_ref(w, bias, xv, 0.25 if use_slope else None))
    return CACHE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("staging", ["float4", "scalar"])
@pytest.mark.parametrize("store", ["planar", "swap"])
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_pw_gemm(ops, name, store, staging, kind):
    L = ops.L
    M, K, B, T, Tp, _, ldo_extra, H = R.GEMM_CASES[name]
    idx, J, swap = list(R.GEMM_CASES).index(name), B * Tp, store == "swap"
    # float4 staging: a pitch of whole float4s with at least four pitch columns, x aligned.  Scalar staging, alternating over the
    # cases: a pitch of 1 or 2 (mod 4), or the float4 pitch with x one float off alignment
    Jp, shift = ceil4(J) + 4, 0
    if staging == "scalar" and idx % 2 == 0:
        Jp = ceil4(J) + 1 + (idx // 2) % 2
    elif staging == "scalar":
        shift = 1
    ldo = M + ldo_extra
    xv, wfrag, bout, slope, ref = gemm_operands(ops, name, kind)
    x = input_planes(ops, xv, Tp, Jp, shift)
    form = int(L.lib().idv_pw_gemm_form(L.i(M), L.i(int(swap)), L.i(Jp), x.ptr()))
    assert form == R.gemm_form(M, swap, Jp, x.addr) and form % 10 == (staging == "float4") and (form // 10) % 10 == swap
    SEEN_GEMM.add(form)

    def call():
        out = Buf(ops, T * B + 4, ldo, SENTINEL) if swap else Buf(ops, M + BEHIND, Jp, SENTINEL)
        L.call("idv_pw_gemm", x.ptr(), L.i(K), L.p(wfrag), L.p(bout), L.p(slope), out.ptr(), L.i(M), L.i(B), L.i(Tp), L.i(Jp), L.i(T),
               L.i(int(swap)), L.i(ldo if swap else 0), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    first = call()
    got = check_rows(first, M, B, T, ldo)[0] if swap else check_planar(first, M, B, T, Tp, J)
    compare(f"idv_pw_gemm {name} {store} form {form}", kind, got, ref, TOL)
    assert torch.equal(first.flat, call().flat), "a second call differs"
    poison(x, K, J)
    assert torch.equal(first.flat, call().flat), "the pitch columns [J, Jp) or planes behind plane K reach the result"


# ----------------------------------------------------------------------------- idv_pw_bf16x3, idv_pw_bf16x3_rows
def bf16_operands(name, kind):
    key = ("bf16", name, kind)
    if key not in CACHE:
        M, K, B, T, Tp = R.BF16_CASES[name]
        g = torch.Generator(device="cuda").manual_seed(2000 + list(R.BF16_CASES).index(name))
        xv, w, bias = draw(kind, (K, B, T), g), draw(kind, (M, K), g, 0.1), draw(kind, (M,), g)
        model = R.split_model(w, xv.reshape(K, B * T)).reshape(M, B, T)
        CACHE[key] = (xv, w, bias, model, R.pw_ref(w, None, xv))
    return CACHE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", ["planar", "rows"])
@pytest.mark.parametrize("name", list(R.BF16_CASES))
def test_pw_bf16x3(ops, name, entry, kind):
    L = ops.L
    M, K, B, T, Tp = R.BF16_CASES[name]
    idx, J = list(R.BF16_CASES).index(name), B * Tp
    Jp = ceil4(J) + 4 if idx % 2 == 0 else J + 1
    xv, w, bias, model, ref = bf16_operands(name, kind)
    no_bias = entry == "planar" and name == R.BF16_NO_BIAS
    ldo = M + 3 if name == R.BF16_WIDE_LDO else M
    addb = (lambda t: t) if no_bias else (lambda t: t + bias.double()[:, None, None])
    wfrag = ops.pack_pw_bf16(w)
    x = input_planes(ops, xv, Tp, Jp)
    tile = int(L.lib().idv_pw_bf16_coltile(L.i(M), L.i(B), L.i(Tp)))
    assert tile == R.bf16_coltile(M, B, Tp)
    SEEN_BF16.add((tile, entry))

    def call():
        kimg = ops.KImage.from_planes(x.ptr(), K, J, Jp, "cuda", pad_to=64)
        if entry == "planar":
            out = Buf(ops, M + BEHIND, Jp, SENTINEL)
            L.call("idv_pw_bf16x3", kimg.ptr(), L.ll(kimg.lo_slots), L.i(K), L.p(wfrag), L.p(None if no_bias else bias), out.ptr(), L.i(M),
                   L.i(B), L.i(Tp), L.i(Jp), L.i(T), L.stream_ptr())
        else:
            out = Buf(ops, T * B + 4, ldo, SENTINEL)
            L.call("idv_pw_bf16x3_rows", kimg.ptr(), L.ll(kimg.lo_slots), L.i(K), L.p(wfrag), L.p(bias), out.ptr(), L.i(M), L.i(ldo),
                   L.i(B), L.i(T), L.i(Tp), L.i(Jp), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    first = call()
    got = check_planar(first, M, B, T, Tp, J) if entry == "planar" else check_rows(first, M, B, T, ldo)[0]
    what = f"idv_pw_bf16x3{'_rows' if entry == 'rows' else ''} {name} tile {tile}"
    compare(what, kind, got, addb(ref if kind == "exact" else model), MODEL_TOL["pw"], whole=addb(ref))
    assert torch.equal(first.flat, call().flat), "a second call differs"
    poison(x, K, J)
    assert torch.equal(first.flat, call().flat), "the pitch columns [J, Jp) or planes behind plane K reach the result"


# ----------------------------------------------------------------------------- the LSTM input projections
def pack_lstm_ih_bf16(ops, H, K, w_re, w_im):
    L = ops.L
    wf = torch.empty(int(L.lib().idv_lstm_ih_bf16_bytes(L.i(H), L.i(K))), dtype=torch.uint8, device="cuda")
    L.call("idv_pack_lstm_ih_bf16", L.p(w_re), L.p(w_im), L.i(H), L.i(K), L.p(wf), L.stream_ptr())
    return wf


def proj_case(ops, kind, entry, H, K, B, T, seed):
    """Both projections: `parts` runs of K planes each in one planar buffer -> G[part][(t, b)][M] with M = 8H (layer 0: every part
    takes the whole stacked matrix) or 4H (layer 1: run = 2 z + s takes weight set s)."""
    L = ops.L
    Tp, J = T + 1, B * (T + 1)
    Jp = ceil4(J) + 4
    parts, M = (2, 8 * H) if entry == "proj" else (4, 4 * H)
    g = torch.Generator(device="cuda").manual_seed(seed)
    ws = draw_lstm(kind, H, K, g)
    xv = draw(kind, (parts, K, B, T), g)
    rows = R.lstm_rows(H).cuda()
    wf32 = torch.cat((ws[0], ws[1]))[rows]                                 # fp32, gate order: what the fragments hold
    W, b = R.lstm_stack(ws[0], ws[1], *ws[2:], H)
    assert torch.equal(W, wf32.double())
    wfrag = pack_lstm_ih_bf16(ops, H, K, ws[0], ws[1])
    _, bias = pack_lstm_ih(ops, H, K, ws)
    sets = (lambda r: slice(0, 8 * H)) if entry == "proj" else (lambda r: slice((r & 1) * 4 * H, ((r & 1) + 1) * 4 * H))
    ref = torch.stack([R.pw_ref(W[sets(r)], b[sets(r)], xv[r]) for r in range(parts)])
    assert torch.equal(ref, R.lstm_proj_ref(W, b, xv) if entry == "proj" else R.lstm_proj1_ref(W, b, xv, H))
    model = torch.stack([R.split_model(wf32[sets(r)], xv[r].reshape(K, B * T)).reshape(M, B, T) + b[sets(r)][:, None, None]
                         for r in range(parts)])
    x = input_planes(ops, xv.reshape(parts * K, B, T), Tp, Jp)
    tile = int(L.lib().idv_pw_bf16_coltile(L.i(M), L.i(B), L.i(Tp)))
    assert tile == R.bf16_coltile(M, B, Tp)
    SEEN_BF16.add((tile, "two-part"))

    def call():
        kimg = ops.KImage.from_planes(x.ptr(), parts * K, J, Jp, "cuda")
        out = Buf(ops, parts * T * B + 4, M, SENTINEL)
        if entry == "proj":
            L.call("idv_lstm_proj_bf16x3", kimg.ptr(), L.ll(kimg.lo_slots), L.i(K), L.p(wfrag), L.p(bias), out.ptr(), L.i(H), L.i(B),
                   L.i(T), L.i(Tp), L.i(Jp), L.stream_ptr())
        else:
            L.call("idv_lstm_proj1_bf16x3", kimg.ptr(), L.ll(kimg.lo_slots), L.p(wfrag), L.p(bias), out.ptr(), L.i(H), L.i(B), L.i(T),
                   L.i(Tp), L.i(Jp), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    first = call()
    got = check_rows(first, M, B, T, M, parts)
    for r in range(parts):
        compare(f"idv_lstm_{entry}_bf16x3 H={H} K={K} B={B} T={T} tile {tile} part {r}", kind, got[r],
                ref[r] if kind == "exact" else model[r], MODEL_TOL[entry], whole=ref[r])
    assert torch.equal(first.flat, call().flat), "a second call differs"
    poison(x, parts * K, J)
    assert torch.equal(first.flat, call().flat), "the pitch columns [J, Jp) or planes behind the last plane reach the result"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.PROJ_CASES))
def test_lstm_proj_bf16x3(ops, name, kind):
    H, K, B, T = R.PROJ_CASES[name]
    proj_case(ops, kind, "proj", H, K, B, T, 3000 + list(R.PROJ_CASES).index(name))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.PROJ1_CASES))
def test_lstm_proj1_bf16x3(ops, name, kind):
    H, B, T = R.PROJ1_CASES[name]
    proj_case(ops, kind, "proj1", H, H, B, T, 4000)


# ----------------------------------------------------------------------------- coverage (last: it reads what the tests above saw)
def test_every_form_was_reached():
    assert SEEN_GEMM == R.GEMM_FORMS, f"idv_pw_gemm forms never launched: {sorted(R.GEMM_FORMS - SEEN_GEMM)}"
    assert SEEN_BF16 == R.BF16_FORMS, f"bf16x3 forms never launched: {sorted(R.BF16_FORMS - SEEN_BF16)}"
