"""ff_encode_yuv without a GPU: the host twin ff_encode_yuv_host against the numpy float32 restatement (tests/yuv_ref.py) byte for byte
over every parameter combination; the knots; the textbook colour-bar codes; neutral greys; the deviation from the float64 true form;
hand-derived siting weights; sanitising; the helpers that the GPU file's tests of tall images stand on; the refusals; the YUV4MPEG2
writer."""
import ctypes as C
import math

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import yuv_ref as R
from yuv_cases import (ALL_COMBINATIONS, DEPTHS, HOST_SIZES, MATRICES, PLANTS, RANGES, SITINGS, TRANSFERS, assert_same, black_planes, blue_on_black,
                       gpu_param_sets, inputs, large_input, name_of, params, planes_below, planted_samples, unshift)

F = np.float32


@pytest.mark.parametrize("combo", ALL_COMBINATIONS, ids=[name_of(c) for c in ALL_COMBINATIONS])
def test_twin_matches_the_restatement_byte_for_byte(combo):
    p = params(*combo)
    for w, h in HOST_SIZES:
        img = inputs(w, h, combo[0])
        if w * h > 100:
            assert img.max() > 50 and (img == 0).sum() == 0 and img.min() < 1e-3
        got = lib.encode_yuv_host(img, p)
        assert got[0].shape == (h, w) and got[1].shape == ((h + 1) // 2, (w + 1) // 2, 2)
        assert lib.yuv_plane_bytes(w, h, p) == (got[0].nbytes, got[1].nbytes)
        assert_same(got, R.encode(img, p), f"{w}x{h}")


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_knots(transfer):
    K = lib.yuv_knots(transfer)
    assert K.dtype == F and K.shape == (4097,)
    assert K[0] == 0 and K[4096] == 1
    assert (np.diff(K.astype(np.float64)) > 0).all()
    want = np.array([R.eotf(transfer, j / 4096) for j in range(4097)], dtype=np.float64).astype(F)
    assert np.array_equal(K.view(np.uint32), want.view(np.uint32))
    # the three curves at a value whose answer is known: 18 % grey codes and the PQ code of 100 nits
    if transfer == T.YUV_TRANSFER_SRGB:
        assert abs(R.eotf(transfer, 0.5) - 0.21404114) < 1e-7
    if transfer == T.YUV_TRANSFER_BT709:
        assert abs(R.eotf(transfer, 0.409) - 0.18) < 1e-3
    if transfer == T.YUV_TRANSFER_PQ:
        assert abs(R.eotf(transfer, 0.508078) - 0.01) < 1e-6


BARS = {  # colour: (r, g, b), (Y, Cb, Cr) under BT.709 LIMITED depth 8
    "black": ((0, 0, 0), (16, 128, 128)),
    "white": ((1, 1, 1), (235, 128, 128)),
    "yellow": ((1, 1, 0), (219, 16, 138)),
    "cyan": ((0, 1, 1), (188, 154, 16)),
    "green": ((0, 1, 0), (173, 42, 26)),
    "magenta": ((1, 0, 1), (78, 214, 230)),
    "red": ((1, 0, 0), (63, 102, 240)),
    "blue": ((0, 0, 1), (32, 240, 118)),
}


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("colour", list(BARS))
def test_textbook_codes(colour, siting):
    rgb, (y, cb, cr) = BARS[colour]
    img = np.empty((4, 8, 3), F)
    img[:] = rgb
    for transfer in (T.YUV_TRANSFER_BT709, T.YUV_TRANSFER_SRGB):  # (a saturated bar is 0 or 1 under either curve)
        luma, chroma = lib.encode_yuv_host(img, params(transfer, siting=siting))
        assert luma.dtype == np.uint8 and (luma == y).all()
        assert (chroma[..., 0] == cb).all() and (chroma[..., 1] == cr).all()
    if colour in ("black", "white"):
        luma, chroma = lib.encode_yuv_host(img, params(depth=10, siting=siting))
        y10 = {"black": 64, "white": 940}[colour]
        assert luma.dtype == np.uint16 and (luma == y10 << 6).all() and (chroma == 512 << 6).all()


def grey_levels(transfer):
    v = (np.arange(4097, dtype=np.float64) / 4096.0)
    if transfer == T.YUV_TRANSFER_PQ:
        v = v * (10000.0 / 203.0)
    return np.ascontiguousarray(np.repeat(v.astype(F)[None, :, None], 3, axis=2))


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_grey_is_neutral(transfer):
    img = grey_levels(transfer)
    assert img.shape == (1, 4097, 3)
    for matrix in MATRICES:
        for range_ in RANGES:
            for depth in DEPTHS:
                for siting in SITINGS:
                    p = params(transfer, matrix, range_, depth, siting)
                    mid = 1 << (depth - 1)
                    # on the restatement alone first: every PIXEL is neutral before the filter, so every sample is
                    y, cb, cr = R.pixel_values(img, p)
                    _, pcb, pcr = R.quantise(y, cb, cr, range_ == T.YUV_RANGE_FULL, depth)
                    assert (pcb == mid).all() and (pcr == mid).all()
                    Y, Cb, Cr = R.codes(img, p)
                    assert (Cb == mid).all() and (Cr == mid).all()
                    assert (np.diff(Y[0]) >= 0).all() and Y[0, 0] == (0 if range_ else 16 << (depth - 8))
                    # then the twin
                    tY, tCb, tCr = unshift(lib.encode_yuv_host(img, p), depth)
                    assert (tCb == mid).all() and (tCr == mid).all() and np.array_equal(tY, Y)


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_deviation_from_the_true_form(transfer, capsys):
    """Against the float64 form with the real pow OETFs and round-half-up every code differs by at most 1.  The bound is derived:
    step 4's e and the true OETF value lie in one cell of 1/4096, so e is off by less than 1/4096 = 0.214 of a 10-bit luma code
    (876 / 4096; 0.053 of an 8-bit one); luma is a convex combination of three such values and a colour difference is a difference
    of two of them divided by Dcb, Dcr > 1.47 and scaled by 896 at most: under 0.3 of a code.  float32 rounding adds under 0.001 of
    a code.  A value less than half a code away from the true one rounds to the same code or to its neighbour."""
    rng = np.random.default_rng(5 + transfer)
    img = np.where(rng.random((32, 64, 3)) < 0.5, rng.random((32, 64, 3)), np.exp(rng.uniform(np.log(1e-4), np.log(60.0), (32, 64, 3)))).astype(F)
    differ = total = 0
    for matrix in MATRICES:
        for range_ in RANGES:
            for depth in DEPTHS:
                for siting in SITINGS:
                    p = params(transfer, matrix, range_, depth, siting)
                    got = unshift(lib.encode_yuv_host(img, p), depth)
                    for g, t in zip(got, R.true_codes(img, p)):
                        d = np.abs(g - t)
                        assert d.max() <= 1, (name_of((transfer, matrix, range_, depth, siting)), int(d.max()))
                        differ += int((d != 0).sum())
                        total += d.size
    with capsys.disabled():
        print(f"\n[yuv deviation] transfer {transfer}: {differ} of {total} codes differ from the true form ({100.0 * differ / total:.3f} %)")
    assert differ < total // 10


# weight of a saturated-blue tap in a chroma sample -> (Cb, Cr) under BT.709 LIMITED depth 8.  Blue is cb = 0.5, cr = -0.0722 / 1.5748 =
# -0.045847: Cb = floor(224 * 0.5 w + 128.5), Cr = floor(128.5 - 224 * 0.045847 w)
WEIGHT_CODES = {0: (128, 128), 0.25: (156, 125), 0.5: (184, 123), 0.75: (212, 120), 1: (240, 118)}


def blue_columns(w, h, columns):
    img = np.zeros((h, w, 3), F)
    for x in columns:
        img[:, x, 2] = 1.0
    return img


def test_weight_codes_by_hand():
    for wgt, (cb, cr) in WEIGHT_CODES.items():
        assert cb == math.floor(224 * 0.5 * wgt + 128.5) and cr == math.floor(128.5 - 224 * (0.0722 / 1.5748) * wgt)


def test_siting_weights():
    def samples(img, siting):
        luma, chroma = lib.encode_yuv_host(img, params(siting=siting))
        assert_same((luma, chroma), R.encode(img, params(siting=siting)))
        assert ((luma == 32) == (img[..., 2] == 1)).all() and ((luma == 16) == (img[..., 2] == 0)).all()
        assert (chroma == chroma[0]).all()  # every row is the same
        return [tuple(int(v) for v in s) for s in chroma[0]]

    W = WEIGHT_CODES
    # 13 wide (7 chroma samples): an even blue column at x = 4 and an odd one at x = 9
    img = blue_columns(13, 4, (4, 9))
    # CENTER: a sample averages its 2 x 2 block, so a blue column has half the weight in the block it falls in
    assert samples(img, T.YUV_SITING_CENTER) == [W[0], W[0], W[0.5], W[0], W[0.5], W[0], W[0]]
    # LEFT: sample X weighs columns 2X-1, 2X, 2X+1 by 1/4, 1/2, 1/4: x = 4 is sample 2's centre; x = 9 is sample 4's right tap and
    # sample 5's left tap
    assert samples(img, T.YUV_SITING_LEFT) == [W[0], W[0], W[0.5], W[0], W[0.25], W[0.25], W[0]]
    # column 0: LEFT's tap at -1 clamps onto it (1/4 + 1/2); CENTER sees it once
    img = blue_columns(13, 4, (0,))
    assert samples(img, T.YUV_SITING_CENTER) == [W[0.5]] + [W[0]] * 6
    assert samples(img, T.YUV_SITING_LEFT) == [W[0.75]] + [W[0]] * 6
    # the last column of an odd width, x = 6 of 7: the taps at x = 7 clamp onto it (CENTER 1/2 + 1/2, LEFT 1/2 + 1/4)
    img = blue_columns(7, 4, (6,))
    assert samples(img, T.YUV_SITING_CENTER) == [W[0]] * 3 + [W[1]]
    assert samples(img, T.YUV_SITING_LEFT) == [W[0]] * 3 + [W[0.75]]
    # ... and of an even width, x = 7 of 8: the last sample's right tap and nobody's left tap
    img = blue_columns(8, 4, (7,))
    assert samples(img, T.YUV_SITING_CENTER) == [W[0]] * 3 + [W[0.5]]
    assert samples(img, T.YUV_SITING_LEFT) == [W[0]] * 3 + [W[0.25]]
    # rows: one blue pixel in the bottom row of an odd height is its block's whole column (the row below clamps onto it)
    img = np.zeros((3, 4, 3), F)
    img[2, 2, 2] = 1.0
    for siting in SITINGS:
        chroma = lib.encode_yuv_host(img, params(siting=siting))[1]
        assert tuple(chroma[1, 1]) == W[0.5] and tuple(chroma[0, 1]) == W[0] and tuple(chroma[1, 0]) == W[0]


@pytest.mark.parametrize("combo", [(T.YUV_TRANSFER_BT709, T.YUV_MATRIX_BT709, T.YUV_RANGE_LIMITED, 8, T.YUV_SITING_LEFT),
                                   (T.YUV_TRANSFER_PQ, T.YUV_MATRIX_BT2020, T.YUV_RANGE_FULL, 10, T.YUV_SITING_CENTER)], ids=name_of)
def test_sanitising(combo):
    p = params(*combo)
    base = (inputs(12, 10, combo[0]) * F(0.01)).astype(F)
    planted, replaced = base.copy(), base.copy()
    where = []
    for i, (bad, stands_for) in enumerate(PLANTS):
        for ch in range(3):
            y, x = 3 * ch + (i & 1), 2 * i + 1
            planted[y, x, ch] = bad
            replaced[y, x, ch] = stands_for
            where.append((y, x))
    assert len(set(where)) == 15
    got = lib.encode_yuv_host(planted, p)
    assert_same(got, lib.encode_yuv_host(replaced, p))
    assert_same(got, R.encode(planted, p))
    # no luma sample of another pixel changes
    untouched = np.ones(base.shape[:2], bool)
    for y, x in where:
        untouched[y, x] = False
    clean = lib.encode_yuv_host(base, p)[0]
    assert np.array_equal(got[0][untouched], clean[untouched])
    assert (got[0][~untouched] != clean[~untouched]).any()


@pytest.mark.parametrize("name", list(gpu_param_sets()))
def test_planted_pixels_below_a_black_top(name):
    """What the GPU file's test of the second tile trip relies on, held here on an image small enough to restate whole: blue pixels
    either side of column 63 | 64 in the last rows of an odd height change exactly planted_samples(), and planes_below() is the
    whole image's planes, for the restatement and for the twin."""
    p = gpu_param_sets()[name]
    w, h, first = 67, 83, 62
    black = black_planes(w, h, p)
    assert_same(black, R.encode(np.zeros((h, w, 3), F), p))
    assert_same(black, lib.encode_yuv_host(np.zeros((h, w, 3), F), p))
    every = [(x, y) for y in (64, 65, 82) for x in (63, 64)]
    for points in [[q] for q in every] + [every]:
        img = blue_on_black(w, h, points)
        want = R.encode(img, p)
        assert_same(planes_below(img, p, first), want, f"{points} restatement")
        assert_same(planes_below(img, p, first, lib.encode_yuv_host), want, f"{points} twin")
        for plane in (0, 1):
            touched = np.argwhere((want[1] != black[1])[..., plane])
            assert {tuple(t) for t in touched.tolist()} == planted_samples(points, p.siting), (points, plane)
        assert {tuple(t) for t in np.argwhere(want[0] != black[0]).tolist()} == {(y, x) for x, y in points}


def test_large_input_holds_every_transfers_knots():
    img = large_input(65, 99)
    assert img.shape == (99, 65, 3) and not img.flags.writeable and img.max() > 50 and img.min() >= 0
    for band, transfer in enumerate(TRANSFERS):
        K = R.knots(transfer) / (F(203) / F(10000)) if transfer == T.YUV_TRANSFER_PQ else R.knots(transfer)
        assert np.isin(img[33 * band:33 * band + 33], K.astype(F)).sum() > 100


def _host_status(w, h, p, img, luma, chroma):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    st = lib.load().ff_encode_yuv_host(w, h, C.byref(p) if p is not None else None, ptr(img), ptr(luma), ptr(chroma))
    return st, lib.load().ff_last_error().decode()


def test_refusals():
    w, h = 6, 4
    img = np.zeros((h, w, 3), F)
    luma, chroma = np.zeros((h, w), np.uint16), np.zeros((2, 3, 2), np.uint16)
    ok = params()
    assert _host_status(w, h, ok, img, luma, chroma)[0] == T.FF_OK
    cases = [
        ((w, h, None, img, luma, chroma), "params"),
        ((w, h, ok, None, luma, chroma), "linear_in"),
        ((w, h, ok, img, None, chroma), "luma"),
        ((w, h, ok, img, luma, None), "chroma"),
        ((0, h, ok, img, luma, chroma), "size"),
        ((w, 0, ok, img, luma, chroma), "size"),
        ((65536, h, ok, img, luma, chroma), "size"),
        ((w, 65536, ok, img, luma, chroma), "size"),
        ((w, h, params(transfer=3), img, luma, chroma), "transfer"),
        ((w, h, params(transfer=-1), img, luma, chroma), "transfer"),
        ((w, h, params(matrix=2), img, luma, chroma), "matrix"),
        ((w, h, params(range_=2), img, luma, chroma), "range"),
        ((w, h, params(siting=2), img, luma, chroma), "siting"),
        ((w, h, params(depth=9), img, luma, chroma), "depth"),
        ((w, h, params(depth=12), img, luma, chroma), "depth"),
        ((w, h, params(depth=0), img, luma, chroma), "depth"),
    ]
    for nits in (0.0, -1.0, 10000.5, float("nan"), float("inf")):
        cases.append(((w, h, params(reference_white_nits=nits), img, luma, chroma), "reference_white_nits"))
    # overlaps: an output on the input, and the two outputs on each other
    flat = np.zeros(h * w * 3, F)
    as_img = flat.reshape(h, w, 3)
    cases.append(((w, h, ok, as_img, flat[-4:].view(np.uint16), chroma), "luma overlaps linear_in"))
    cases.append(((w, h, ok, as_img, luma, flat[:4].view(np.uint16)), "chroma overlaps linear_in"))
    both = np.zeros(64, np.uint8)
    cases.append(((w, h, ok, img, both[:24], both[23:]), "luma overlaps chroma"))
    for args, field in cases:
        st, msg = _host_status(*args)
        assert st == T.FF_ERR_INVALID_ARG and field in msg and msg.startswith("ff_encode_yuv_host:"), (field, st, msg)
    st, msg = _host_status(w, h, ok, img, both[:24], both[24:])  # (adjacent is not overlapping)
    assert st == T.FF_OK
    # the device entry point names a missing state before anything else
    L = lib.load()
    st = L.ff_encode_yuv(None, w, h, C.byref(ok), img.ctypes.data, 0, luma.ctypes.data, chroma.ctypes.data, 0)
    assert st == T.FF_ERR_INVALID_ARG and "state" in L.ff_last_error().decode()
    # the helpers
    with pytest.raises(lib.FireflyError, match="depth"):
        lib.yuv_plane_bytes(4, 4, params(depth=9))
    with pytest.raises(lib.FireflyError, match="transfer"):
        lib.yuv_knots(3)
    assert L.ff_yuv_knots(0, None) == T.FF_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        lib.yuv_params(gamma=2.2)
    assert lib.yuv_plane_bytes(5, 3, params(depth=10)) == (30, 24) and lib.yuv_plane_bytes(5, 3) == (15, 12)


def test_params_defaults():
    p = lib.yuv_params()
    assert (p.transfer, p.matrix, p.range, p.depth, p.siting, p.reference_white_nits) == (
        T.YUV_TRANSFER_BT709, T.YUV_MATRIX_BT709, T.YUV_RANGE_LIMITED, 8, T.YUV_SITING_LEFT, 203.0)


def parse_y4m(data):
    """-> (header fields, [frames of (Y, Cb, Cr) integer planes])."""
    end = data.index(b"\n")
    fields = data[:end].decode().split(" ")
    assert fields[0] == "YUV4MPEG2"
    tags = {f[0]: f[1:] for f in fields[1:]}
    w, h = int(tags["W"]), int(tags["H"])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    dtype = "<u2" if tags["C"] == "420p10" else np.uint8
    size = np.dtype(dtype).itemsize
    frames, pos = [], end + 1
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n"
        pos += 6
        planes = []
        for n, shape in ((w * h, (h, w)), (cw * ch, (ch, cw)), (cw * ch, (ch, cw))):
            planes.append(np.frombuffer(data, dtype=dtype, count=n, offset=pos).reshape(shape).astype(np.int64))
            pos += n * size
        frames.append(planes)
    return fields, frames


@pytest.mark.parametrize("depth,siting,range_,colourspace", [(8, T.YUV_SITING_LEFT, T.YUV_RANGE_LIMITED, "C420mpeg2"), (8, T.YUV_SITING_CENTER, T.YUV_RANGE_FULL, "C420jpeg"),
                                                            (10, T.YUV_SITING_LEFT, T.YUV_RANGE_LIMITED, "C420p10")])
def test_save_y4m(tmp_path, depth, siting, range_, colourspace):
    w, h = 7, 5
    transfer = T.YUV_TRANSFER_PQ if depth == 10 else T.YUV_TRANSFER_BT709
    p = params(transfer, range_=range_, depth=depth, siting=siting)
    frames = [lib.encode_yuv_host(inputs(w, h, transfer, seed=s), p) for s in (1, 2)]
    path = tmp_path / "two.y4m"
    lib.save_y4m(path, *frames[0], p)
    lib.save_y4m(path, *frames[1], p, append=True)
    fields, parsed = parse_y4m(path.read_bytes())
    assert fields[1:3] == [f"W{w}", f"H{h}"] and colourspace in fields
    assert f"XCOLORRANGE={'FULL' if range_ else 'LIMITED'}" in fields
    assert len(parsed) == 2
    for (luma, chroma), (Y, Cb, Cr) in zip(frames, parsed):
        eY, eCb, eCr = unshift((luma, chroma), depth)
        assert np.array_equal(Y, eY) and np.array_equal(Cb, eCb) and np.array_equal(Cr, eCr)
        assert Y.max() <= (1 << depth) - 1 and len(np.unique(Y)) > 4
    # a second stream over the first starts again; a path that cannot be written is FF_ERR_IO
    lib.save_y4m(path, *frames[0], p)
    assert len(parse_y4m(path.read_bytes())[1]) == 1
    with pytest.raises(lib.FireflyError) as e:
        lib.save_y4m(tmp_path / "no_such_dir" / "x.y4m", *frames[0], p)
    assert e.value.status == T.FF_ERR_IO
