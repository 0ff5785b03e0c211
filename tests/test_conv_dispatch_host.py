"""CPU: which direct-kernel instantiation sda_conv_igemm launches (conv_pick and the variant table in csrc/conv_igemm.hip).

tests/golden/conv_dispatch.json was recorded from the if / switch ladder that chose the instantiation before conv_pick existed: a
host build of that code which noted, in place of launching, the kernel symbol, the planned geometry, the dynamic LDS and the
return code.  The pick function, called through libsda_emu.so with the four environment switches as arguments, must give the same
answer on every case, name table rows only, and the cases must reach every row of the table."""
import ctypes

import pytest

from sda_amd import build as sbuild
from sda_amd._lib import ConvDesc
from tests.util import conv_dispatch_desc, load_conv_dispatch


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_conv_igemm_pick.restype = ctypes.c_int
    lib.sda_conv_igemm_pick.argtypes = [ctypes.POINTER(ConvDesc)] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)]
    lib.sda_conv_igemm_variants.restype = ctypes.c_int
    lib.sda_conv_igemm_variants.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


@pytest.fixture(scope='module')
def cases():
    return load_conv_dispatch()


def variants(emu):
    n = emu.sda_conv_igemm_variants(None, 0)
    buf = (ctypes.c_int * (8 * n))()
    assert emu.sda_conv_igemm_variants(buf, n) == n
    return [tuple(buf[8 * i:8 * i + 8]) for i in range(n)]


def pick(emu, c):
    out = (ctypes.c_int * 16)()
    rc = emu.sda_conv_igemm_pick(ctypes.byref(conv_dispatch_desc(c)), *c['switches'], out)
    return rc, tuple(out[:8]), tuple(out[8:])


def test_pick_matches_the_recorded_dispatch(emu, cases):
    assert len(cases) > 500
    for c in cases:
        rc, p, geom = pick(emu, c)
        assert rc == c['rc'], c
        if rc == 0:
            assert (p, geom) == (c['pick'], c['geom']), c


def test_the_cases_reach_every_variant_and_name_no_other(emu, cases):
    table = variants(emu)
    assert len(table) == len(set(table)) == 93                           # 85 wave-specialised instantiations, 8 of the v1 kernel
    picked = {c['pick'] for c in cases if c['rc'] == 0}
    assert picked <= set(table), picked - set(table)
    assert set(table) <= picked, set(table) - picked
    # ... and without any switch, on a launch no other kernel family takes (what test_gpu_ops.py runs on the device)
    plain = {c['pick'] for c in cases if c['rc'] == 0 and c['direct'] and c['switches'] == (0, 0, 1, 1) and not c['misalign']}
    assert plain == set(table), set(table) - plain


def test_null_descriptor_is_a_bad_argument(emu):
    out = (ctypes.c_int * 16)()
    assert emu.sda_conv_igemm_pick(None, 0, 0, 1, 1, out) == -1
