"""The one path of the single-image filters (gpupathtracer_amd.tracer._filter), without a GPU: what it refuses, with the error
texts the methods had when each carried its own copy of the dispatch, and what it hands to the C call for a host array."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, tracer
from gpupathtracer_amd import types as T

SINGLE_IMAGE = [  # method, extra positional arguments, its parameter struct
    ("sharpen", (), T.FfSharpenParams),
    ("lens", (), T.FfLensParams),
    ("resize", (8, 6), T.FfResizeParams),
    ("local_tonemap", (), T.FfLocalTonemapParams),
    ("color_grade", (), T.FfGradeParams),
]


class HostTensor:
    """What the dispatch sees of a torch tensor that is not on the device."""
    shape, dtype, is_cuda = (4, 5, 3), "float32", False

    def data_ptr(self):
        return 0

    def is_contiguous(self):
        return True


@pytest.fixture
def unbound():
    """A Tracer without an FfState (no ff_create, no library handle): any C call through it raises AttributeError."""
    return object.__new__(lib.Tracer)


@pytest.mark.parametrize("method,extra,params", SINGLE_IMAGE)
def test_a_tensor_that_is_not_on_the_device_is_refused(unbound, method, extra, params):
    with pytest.raises(ValueError) as e:
        getattr(unbound, method)(HostTensor(), *extra, p=params())
    assert str(e.value) == f"{method}: radiance must be a contiguous [H,W,3] float32 tensor on the device"


@pytest.mark.parametrize("method,extra,params", SINGLE_IMAGE)
def test_a_host_array_of_the_wrong_shape_is_refused_before_the_call(unbound, method, extra, params):
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 5, 4), np.float32)):
        with pytest.raises(ValueError) as e:
            getattr(unbound, method)(bad, *extra, p=params())
        assert str(e.value) == f"{method}: radiance must be [H,W,3]"


def test_the_other_filters_validators_are_first_too(unbound):
    rad, plane = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.float32)
    cases = [
        (lambda: unbound.display(plane, p=T.FfDisplayParams()), "display: radiance must be [H,W,3]"),
        (lambda: unbound.encode_yuv(plane, p=T.FfYuvParams()), "encode_yuv: radiance must be [H,W,3]"),
        (lambda: unbound.motion_blur(rad, plane, plane, p=T.FfMotionBlurParams()),
         "motion_blur: radiance must be [H,W,3], motion [H,W,2] and depth [H,W]"),
        (lambda: unbound.depth_of_field(rad, (plane, plane), T.FfCamera(), p=T.FfDofParams()),
         "depth_of_field: radiance and position must be [H,W,3] and depth [H,W]"),
        (lambda: unbound.despeckle(rad, (None, plane), p=T.FfDespeckleParams()), "despeckle: radiance, albedo and ids must be [H,W,3]"),
        (lambda: unbound.taa(plane, {"position": rad, "ids": rad}, T.FfCamera(), p=T.FfTaaParams()),
         "taa: radiance must be [H,W,3] and the G-buffer of the same size"),
    ]
    for call, message in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message


def _recorded(radiance, **kw):
    """tracer._filter on a host array with a C call that only records its arguments -> (the arguments, what _filter returned)."""
    seen = {}

    def call(w, h, src, tail):
        seen.update(w=w, h=h, src=src, tail=tail)
        return T.FF_OK
    return seen, tracer._filter("probe", radiance, call, **kw)


def test_host_array_call_gets_size_pointers_and_zero_flags():
    rad = np.arange(4 * 5 * 3, dtype=np.float32).reshape(4, 5, 3)
    seen, (rgb8, out) = _recorded(rad, want_rgb8=True, want_out=True)
    assert (seen["w"], seen["h"], seen["src"]) == (5, 4, rad.ctypes.data)
    flag, rgb8_ptr, flag2, out_ptr, flag3 = seen["tail"]
    assert (flag, flag2, flag3) == (0, 0, 0) and rgb8_ptr.value == rgb8.ctypes.data and out_ptr.value == out.ctypes.data
    assert rgb8.shape == out.shape == (4, 5, 3) and rgb8.dtype == np.uint8 and out.dtype == np.float32
    # an output that is not wanted is None, and so is its pointer
    seen, (rgb8, out) = _recorded(rad, want_rgb8=False, want_out=True)
    assert rgb8 is None and seen["tail"][1] is None and out is not None
    seen, (rgb8, out) = _recorded(rad, want_rgb8=True, want_out=False)
    assert out is None and seen["tail"][3] is None and rgb8 is not None
    # a list is converted; resize's outputs have their own size
    seen, (rgb8, out) = _recorded(rad.tolist(), want_rgb8=True, want_out=True, out_size=(2, 7))
    assert (seen["w"], seen["h"]) == (5, 4) and rgb8.shape == out.shape == (2, 7, 3)


def test_in_place_on_a_host_array_works_on_a_copy():
    rad = np.arange(4 * 5 * 3, dtype=np.float32).reshape(4, 5, 3)
    before = rad.copy()
    seen, (rgb8, out) = _recorded(rad, want_rgb8=True, want_out=True, in_place=True)
    # radiance_out is radiance_in in the call, neither is the caller's array, and the copy holds the input
    assert seen["src"] == seen["tail"][3].value == out.ctypes.data != rad.ctypes.data
    assert np.array_equal(out, before) and np.array_equal(rad, before)
    # without the float output the caller's array is the source
    seen, (rgb8, out) = _recorded(rad, want_rgb8=True, want_out=False, in_place=True)
    assert out is None and seen["src"] == rad.ctypes.data and seen["tail"][3] is None


def test_a_failing_call_raises_the_status(ff):
    with pytest.raises(ff.FireflyError) as e:
        tracer._filter("probe", np.zeros((2, 2, 3), np.float32), lambda w, h, src, tail: T.FF_ERR_INVALID_ARG, True, True)
    assert e.value.status == T.FF_ERR_INVALID_ARG
