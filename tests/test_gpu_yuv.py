"""ff_encode_yuv on the GPU: byte for byte against the numpy float32 restatement (tests/yuv_ref.py) and against the host twin over image
sizes around the lane's 4 x 2 block and the kernel's tiles, under four parameter sets that launch the four instantiations
yuv_kernel<8 | 10, LEFT | CENTER>; every parameter combination at an odd height on the scalar and on the vector path (the latter also
through 16-byte-aligned device tensors); images of more than 2 048 tiles, where workgroups take a second trip of the tile loop, whole
and with planted pixels at the tile seam of that trip; planted pixels at every power-of-two seam; NaN, negative and huge values
where lanes and tiles meet; buffer kinds and misaligned device buffers, the staging regrown, the knots of another transfer, refused
overlaps; isolation from the other entry points; and the chain render -> ff_display (display_out) -> ff_encode_yuv on a real 1-spp
frame."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import yuv_ref as R
from yuv_cases import (ALL_COMBINATIONS, COMBINATION_SIZES, GPU_SIZES, MEET_COLUMNS, MEET_ROWS, PLANTS, SEAM_COLUMNS, SEAM_ROWS, SEAM_SIZE, TALL_PLANT_COLUMNS,
                       TALL_PLANT_ROWS, TALL_SIZES, WIDE_SIZE, assert_same, black_planes, blue_on_black, gpu_param_sets, inputs, large_input, name_of,
                       params, planes_below, planted_samples, unshift)

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)
SETS = gpu_param_sets()


def check_all_three(tracer, img, p, what=""):
    got = tracer.encode_yuv(img, p)
    assert_same(got, R.encode(img, p), what + " kernel vs restatement")
    assert_same(got, lib.encode_yuv_host(img, p), what + " kernel vs twin")
    return got


def encode_on_aligned_tensors(tracer, img, p):
    """The planes through the device-tensor entry point, with the three buffers' 16-byte alignment asserted: at a width that is a
    multiple of 4 this call takes the kernel's whole-dword path (YuvArgs::vec), whatever the staging of host buffers does."""
    import torch
    d_img = torch.from_numpy(np.array(img)).cuda()
    d_luma, d_chroma = tracer.encode_yuv_device(d_img, p)
    for t in (d_img, d_luma, d_chroma):
        assert t.data_ptr() % 16 == 0
    return d_luma.cpu().numpy(), d_chroma.cpu().numpy()


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("w,h", GPU_SIZES, ids=[f"{w}x{h}" for w, h in GPU_SIZES])
def test_reference_and_twin_parity_byte_for_byte(tracer, w, h, name):
    p = SETS[name]
    img = inputs(w, h, p.transfer)
    luma, chroma = check_all_three(tracer, img, p, f"{name} {w}x{h}")
    if w * h >= 64 * 16:
        assert len(np.unique(luma)) > 32 and len(np.unique(chroma)) > 32
    assert_same(encode_on_aligned_tensors(tracer, img, p), (luma, chroma), f"{name} {w}x{h} aligned device tensors")


@pytest.mark.parametrize("combo", ALL_COMBINATIONS, ids=[name_of(c) for c in ALL_COMBINATIONS])
def test_every_combination_on_the_device(tracer, combo):
    """Every transfer x matrix x range x depth x siting the host file runs, at an odd height over two tile columns: 67 x 19 on the
    scalar path, 68 x 19 on the vector path (host buffers staged 16-byte aligned, and aligned device tensors)."""
    p = params(*combo)
    for w, h in COMBINATION_SIZES:
        img = inputs(w, h, combo[0])
        got = check_all_three(tracer, img, p, f"{name_of(combo)} {w}x{h}")
        assert_same(encode_on_aligned_tensors(tracer, img, p), got, f"{name_of(combo)} {w}x{h} aligned device tensors")


@pytest.mark.parametrize("name", list(SETS))
def test_seams(tracer, name):
    """Saturated-blue pixels on a black image at columns 63, 64, 65, 127, 128 and rows 15, 16, 17: a LEFT tap at column 2X - 1 crosses
    every power-of-two tile edge up to 64 x 16 (the kernel's lanes own 4 x 2 blocks, its tiles are 64 x 32), and every planted pixel
    must show in its chroma sample (and, for an odd column under LEFT, in the next one too)."""
    p = SETS[name]
    w, h = SEAM_SIZE
    img = np.zeros((h, w, 3), F)
    for y in SEAM_ROWS:
        for x in SEAM_COLUMNS:
            img[y, x, 2] = 1.0
    black = unshift(check_all_three(tracer, np.zeros((h, w, 3), F), p), p.depth)
    _, cb, cr = unshift(check_all_three(tracer, img, p, name), p.depth)
    assert (black[1] == black[1][0, 0]).all() and (black[2] == black[2][0, 0]).all()
    for y in SEAM_ROWS:
        for x in SEAM_COLUMNS:
            assert cb[y // 2, x // 2] != black[1][0, 0], (x, y)
            if p.siting == T.YUV_SITING_LEFT and x % 2 == 1:
                assert cb[y // 2, x // 2 + 1] != black[1][0, 0], (x, y)
    # one planted pixel at a time: the neighbour's column really comes from the neighbouring lane or tile
    for x in SEAM_COLUMNS:
        one = np.zeros((h, w, 3), F)
        one[16, x, 2] = 1.0
        _, cb1, _ = unshift(check_all_three(tracer, one, p, f"{name} x={x}"), p.depth)
        touched = np.argwhere(cb1 != black[1][0, 0])
        want = {(8, x // 2)} | ({(8, x // 2 + 1)} if p.siting == T.YUV_SITING_LEFT and x % 2 == 1 else set())
        assert {tuple(t) for t in touched.tolist()} == want, (x, touched.tolist())


TALL_IDS = [f"{w}x{h}" for w, h in TALL_SIZES]


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("w,h", TALL_SIZES, ids=TALL_IDS)
def test_more_tiles_than_workgroups(tracer, w, h, name):
    """2 x 1025 tiles on 2 048 workgroups: workgroups 0 and 1 take a second trip of the tile loop, over a last tile row of 19 rows
    (65 wide on the scalar path, 68 wide on the vector path).  The whole planes against the restatement and the twin."""
    luma, chroma = check_all_three(tracer, large_input(w, h), SETS[name], f"{name} {w}x{h}")
    assert len(np.unique(luma[32768:])) > 32 and len(np.unique(chroma[16384:])) > 32


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("w,h", TALL_SIZES, ids=TALL_IDS)
def test_seam_of_the_second_trip(tracer, w, h, name):
    """Saturated-blue pixels on a black image either side of the tile seam 63 | 64 in rows 32768, 32769 (the first lane rows of the
    second trip) and 32786 (the last row, repeated as the row below it), one at a time and together: exactly the planted pixels'
    chroma samples differ from black - under LEFT sample 32 too for column 63, which the second tile's edge lanes load themselves -
    and the planes are the restatement's and the twin's (of the rows from 32766 on; black above, tests/test_yuv_host.py)."""
    p = SETS[name]
    black = black_planes(w, h, p)
    assert_same(tracer.encode_yuv(np.zeros((h, w, 3), F), p), black, f"{name} black")
    every = [(x, y) for y in TALL_PLANT_ROWS for x in TALL_PLANT_COLUMNS]
    for points in [[q] for q in every] + [every]:
        img = blue_on_black(w, h, points)
        got = tracer.encode_yuv(img, p)
        assert_same(got, planes_below(img, p, 32766), f"{name} {points} kernel vs restatement")
        assert_same(got, planes_below(img, p, 32766, lib.encode_yuv_host), f"{name} {points} kernel vs twin")
        for plane in (0, 1):
            touched = np.argwhere((got[1] != black[1])[..., plane])
            assert {tuple(t) for t in touched.tolist()} == planted_samples(points, p.siting), (points, plane, touched.tolist())


def test_a_whole_tile_row_of_second_trips(tracer):
    """65535 x 65: 1024 x 3 tiles, so every workgroup of the first tile row comes back for the third."""
    w, h = WIDE_SIZE
    name = "p010-pq-bt2020-limited-left"
    luma, chroma = check_all_three(tracer, large_input(w, h), SETS[name], f"{name} {w}x{h}")
    assert len(np.unique(luma[64:])) > 32 and len(np.unique(chroma[32:])) > 32


@pytest.mark.parametrize("name", list(SETS))
def test_sanitising_where_lanes_and_tiles_meet(tracer, name):
    """NaN, -1, -Inf, +Inf and 1e30 in each channel at every pixel where two lanes or two tiles meet - columns 3 | 4, 63 | 64,
    127 | 128 and the last one, rows 1 | 2, 31 | 32 and the last one - and down the whole of column 63, which the second tile's edge
    lanes load and sanitise themselves under LEFT.  The columns left and right of a seam are planted in images of their own, so that
    no chroma sample hides one plant behind another.  The kernel equals the restatement, the twin, and itself on the image with the
    stand-in values written in; no luma sample of an unplanted pixel changes."""
    p = SETS[name]
    w, h = SEAM_SIZE
    base = (inputs(w, h, p.transfer) * F(0.01)).astype(F)
    clean = tracer.encode_yuv(base, p)[0]
    groups = [[(x, y) for y in MEET_ROWS for x in MEET_COLUMNS[0::2]], [(x, y) for y in MEET_ROWS for x in MEET_COLUMNS[1::2]], [(63, y) for y in range(h)]]
    assert {x for g in groups[:2] for x, _ in g} == set(MEET_COLUMNS) and MEET_COLUMNS[-1] == w - 1 and MEET_ROWS[-1] == h - 1
    for bad, stands_for in PLANTS:
        for ch in range(3):
            for places in groups:
                planted, replaced = base.copy(), base.copy()
                untouched = np.ones((h, w), bool)
                for x, y in places:
                    planted[y, x, ch] = bad
                    replaced[y, x, ch] = stands_for
                    untouched[y, x] = False
                got = check_all_three(tracer, planted, p, f"{name} {bad} in channel {ch}")
                assert_same(got, tracer.encode_yuv(replaced, p), f"{name} {bad} in channel {ch}: planted vs replaced")
                assert np.array_equal(got[0][untouched], clean[untouched])
                assert (got[0][~untouched] != clean[~untouched]).any()


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("w,h", [(68, 18), (68, 19)], ids=["68x18", "68x19"])
def test_misaligned_device_buffers(tracer, w, h, name):
    """Device buffers that are aligned to their samples only, at a width that is a multiple of 4: the input 4 bytes, luma one sample
    (1 byte for NV12, 2 for P010) and chroma three samples (3 and 6 bytes) past 16-byte alignment.  The planes are the aligned
    call's, and every byte around them stays zero."""
    import torch
    p = SETS[name]
    img = inputs(w, h, p.transfer)
    want = encode_on_aligned_tensors(tracer, img, p)
    sample = 1 if p.depth == 8 else 2
    lb, cb = lib.yuv_plane_bytes(w, h, p)
    big = torch.zeros(h * w * 3 + 8, dtype=torch.float32, device="cuda")
    big[1:1 + h * w * 3] = torch.from_numpy(np.array(img)).cuda().reshape(-1)
    b_luma = torch.zeros(lb + 32, dtype=torch.uint8, device="cuda")
    b_chroma = torch.zeros(cb + 32, dtype=torch.uint8, device="cuda")
    for t in (big, b_luma, b_chroma):
        assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    lo, co = sample, 3 * sample
    vp = C.c_void_p
    lib.check(lib.load().ff_encode_yuv(tracer._state, w, h, C.byref(p), vp(big.data_ptr() + 4), 1, vp(b_luma.data_ptr() + lo), vp(b_chroma.data_ptr() + co), 1))
    luma, chroma = b_luma.cpu().numpy(), b_chroma.cpu().numpy()
    assert_same((luma[lo:lo + lb].view(want[0].dtype).reshape(want[0].shape), chroma[co:co + cb].view(want[1].dtype).reshape(want[1].shape)), want, name)
    assert not luma[:lo].any() and not luma[lo + lb:].any() and not chroma[:co].any() and not chroma[co + cb:].any()
    assert np.array_equal(big.cpu().numpy()[1:1 + h * w * 3].view(np.uint32), img.reshape(-1).view(np.uint32))


def test_buffer_kinds_regrowth_and_transfers(tracer):
    import torch
    p = SETS["nv12-bt709-limited-left"]
    hdr = SETS["p010-pq-bt2020-limited-left"]
    w, h = 68, 18
    img = inputs(w, h)
    host = check_all_three(tracer, img, p)
    # device tensors in and out
    d_img = torch.from_numpy(np.array(img)).cuda()
    d_luma, d_chroma = tracer.encode_yuv_device(d_img, p)
    assert d_luma.is_cuda and d_chroma.is_cuda and d_luma.dtype == torch.uint8
    assert_same((d_luma.cpu().numpy(), d_chroma.cpu().numpy()), host)
    assert np.array_equal(d_img.cpu().numpy().view(np.uint32), img.view(np.uint32))  # (the input is left alone)
    # into given tensors, at depth 10 (the knots of another transfer are uploaded)
    host10 = check_all_three(tracer, img, hdr)
    g_luma = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    g_chroma = torch.zeros((h // 2, w // 2, 2), dtype=torch.int16, device="cuda")
    out = tracer.encode_yuv_device(d_img, hdr, g_luma, g_chroma)
    assert out[0] is g_luma and out[1] is g_chroma
    assert_same((g_luma.cpu().numpy(), g_chroma.cpu().numpy()), host10)
    # ... and back to the first transfer, and the third
    assert_same(tracer.encode_yuv(img, p), host)
    check_all_three(tracer, img, SETS["nv12-srgb-full-center"])
    # mixed: a device input with host outputs, a host input with device outputs, through the raw entry point
    lib_ = lib.load()
    vp = C.c_void_p
    m_luma, m_chroma = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2, 2), np.uint8)
    lib.check(lib_.ff_encode_yuv(tracer._state, w, h, C.byref(p), vp(d_img.data_ptr()), 1, m_luma.ctypes.data, m_chroma.ctypes.data, 0))
    assert_same((m_luma, m_chroma), host)
    d_luma.zero_()
    d_chroma.zero_()
    torch.cuda.synchronize()
    lib.check(lib_.ff_encode_yuv(tracer._state, w, h, C.byref(p), img.ctypes.data, 0, vp(d_luma.data_ptr()), vp(d_chroma.data_ptr()), 1))
    assert_same((d_luma.cpu().numpy(), d_chroma.cpu().numpy()), host)
    # buffers that are only 4-byte (1-byte) aligned: the scalar path at a width that is a multiple of 4
    big = torch.zeros(h * w * 3 + 8, dtype=torch.float32, device="cuda")
    big[1:1 + h * w * 3] = d_img.reshape(-1)
    b_luma = torch.zeros(h * w + 8, dtype=torch.uint8, device="cuda")
    b_chroma = torch.zeros(h * w // 2 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib.check(lib_.ff_encode_yuv(tracer._state, w, h, C.byref(p), vp(big.data_ptr() + 4), 1, vp(b_luma.data_ptr() + 1), vp(b_chroma.data_ptr() + 3), 1))
    assert_same((b_luma.cpu().numpy()[1:1 + h * w].reshape(h, w), b_chroma.cpu().numpy()[3:3 + h * w // 2].reshape(h // 2, w // 2, 2)), host)
    assert (b_luma.cpu().numpy()[[0, -7]] == 0).all() and (b_chroma.cpu().numpy()[[0, 1, 2, -5]] == 0).all()
    # a second, larger call after a small one (the staging is regrown), then small again
    for size in ((130, 35), (5, 2), (67, 19)):
        check_all_three(tracer, inputs(*size), p)
    # an output on the input or on the other output is refused on the host: nothing is launched, nothing is written
    guard = torch.full((h * w,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    src = d_img.data_ptr()
    for luma_ptr, chroma_ptr, words in [(src, guard.data_ptr(), "luma overlaps linear_in"), (src + 12 * w * h - 1, guard.data_ptr(), "luma overlaps linear_in"),
                                        (guard.data_ptr(), src + 64, "chroma overlaps linear_in"),
                                        (guard.data_ptr(), guard.data_ptr() + h * w - 1, "luma overlaps chroma")]:
        st = lib_.ff_encode_yuv(tracer._state, w, h, C.byref(p), vp(src), 1, vp(luma_ptr), vp(chroma_ptr), 1)
        assert st == T.FF_ERR_INVALID_ARG and words in lib_.ff_last_error().decode()
    assert (guard.cpu().numpy() == 7).all()
    assert np.array_equal(d_img.cpu().numpy().view(np.uint32), img.view(np.uint32))
    # the parameter checks run before any device work, with a state
    for field, value in [("transfer", 5), ("matrix", -1), ("range", 3), ("depth", 16), ("siting", 2), ("reference_white_nits", 0.0)]:
        q = lib.yuv_params(**{field: value})
        st = lib_.ff_encode_yuv(tracer._state, w, h, C.byref(q), vp(src), 1, vp(guard.data_ptr()), vp(d_chroma.data_ptr()), 1)
        assert st == T.FF_ERR_INVALID_ARG and field in lib_.ff_last_error().decode()
    assert (guard.cpu().numpy() == 7).all()


def test_encode_yuv_is_not_a_frame(tracer):
    w, h = 96, 64
    scene = scenes.cornell_wahoo_scene()
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), **C2_POSE)
    prm = lib.render_params(w, h, 6, 1, 42)
    tracer.upload_scene(scene)
    first = tracer.render(cam, prm)
    second = tracer.render(cam, prm)           # (the camera is at rest: served from the stored primary hits)
    st, name = tracer.stats(), tracer.kernel_name()
    auto = lib.display_params(flags=T.DISPLAY_AUTO_EXPOSURE, encoding=T.ENCODE_LINEAR)
    shown = tracer.display(second[1], auto)[1]
    disp = tracer.display_state()

    def snapshot():
        s = tracer.stats()
        return {f: getattr(s, f) for f, _ in s._fields_}
    before = snapshot()
    for p in SETS.values():
        check_all_three(tracer, shown, p)
    assert snapshot() == before and tracer.kernel_name() == name
    after = tracer.display_state()
    assert after[:2] == disp[:2] and np.array_equal(after[2], disp[2])
    # the next adapting display call starts from the same exposure as without the encode in between
    third = tracer.render(cam, prm)
    assert np.array_equal(third[0], second[0]) and np.array_equal(third[1].view(np.uint32), second[1].view(np.uint32))
    assert np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))
    s3 = tracer.stats()
    assert (s3.rays_answered, s3.rays_traced, s3.flags, s3.kernel_launches) == (st.rays_answered, st.rays_traced, st.flags, st.kernel_launches)


def test_chain_on_a_real_frame(tracer):
    """A 64 x 36 1-spp frame of the Cornell box with next-event estimation through ff_display's display_out (ACES, linear semantics)
    into NV12, and through the PQ / BT.2020 / P010 path as radiance: the planes equal the restatement applied to the downloaded
    display_out, and the luma plane is an image."""
    w, h = 64, 36
    tracer.upload_scene(scenes.cornell_mirror_scene())
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 5.0), **C2_POSE)
    rad = tracer.render(cam, lib.render_params(w, h, 8, 1, seed=11, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    shown = tracer.display(rad, lib.display_params(encoding=T.ENCODE_LINEAR))[1]
    assert shown.min() >= 0 and shown.max() <= 1
    for name, img in (("nv12-bt709-limited-left", shown), ("nv12-srgb-full-center", shown), ("p010-pq-bt2020-limited-left", rad),
                      ("p010-bt709-bt2020-full-center", shown)):
        luma, chroma = check_all_three(tracer, img, SETS[name], name)
        print(f"{name}: {len(np.unique(luma))} luma codes, {len(np.unique(chroma))} chroma codes")
        assert len(np.unique(luma)) > 8 and len(np.unique(chroma)) > 2
