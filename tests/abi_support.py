"""What the tests that need no GPU share (the six tests/test_*_abi.py, tests/test_kernel_resources.py
and tests/test_kernel_copies.py): the repository root with tools/ on the path, the return codes, one
camera that passes validate_camera, and the asserts every entry point repeats.  A helper module, not
a test: pytest does not rewrite its asserts, so each carries its own message."""
import ctypes as C
import os
import sys

import rtzig
from rtzig.abi import RT_ERR_INVALID, RT_OK, RtCamera  # noqa: F401 (the codes are re-exported)
from rtzig.lib import EXPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_build  # noqa: E402


def resources(source):
    """kernel_build.resources: per kernel of a csrc file, the compiler's register and memory figures."""
    return kernel_build.resources(source)


def vp(buf):
    return C.cast(buf, C.c_void_p)


def cam_of(w=4, h=3):
    """A camera of w x h pixels that passes validate_camera (finite vectors, a scale, a hit interval),
    whose du x dv is not 0 and whose centre lies off its image plane."""
    cam = RtCamera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.bounce_max = w, h, 1, 1
    cam.pixel_samples_scale = 1.0
    cam.t_min, cam.t_max = 1e-3, float("inf")
    for k in range(3):
        cam.center[k] = 0.0
        cam.pixel0[k] = (-0.5, 0.5, -1.0)[k]
        cam.du[k] = (0.25, 0.0, 0.0)[k]
        cam.dv[k] = (0.0, -0.25, 0.0)[k]
    return cam


def assert_invalid(rc, word):
    """The call returned RT_ERR_INVALID and rt_last_error names what it refused."""
    assert rc == RT_ERR_INVALID, "returned %r, not RT_ERR_INVALID" % (rc,)
    msg = rtzig.load().rt_last_error()
    assert word in msg, "%r not in rt_last_error() %r" % (word, msg)


def assert_bound(name, n_args):
    """The symbol is exported, bound, returns int and takes n_args arguments."""
    assert name in EXPORTED, "%s is not in rtzig.lib.EXPORTED" % name
    fn = getattr(rtzig.load(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == n_args, \
        "%s: restype %r, %d arguments (int and %d wanted)" % (name, fn.restype, len(fn.argtypes), n_args)
