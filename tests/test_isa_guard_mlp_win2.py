"""CPU build-time guard for the two-fragment window kernels of csrc/mlp1d.hip (mlp_win2_*: windows of 17 .. 32 values), the rule
tests/test_isa_guard_mlp.py holds the other eight whole-MLP kernels to: no spill, no scratch access, inside the register file and the LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import isa_guard as G  # noqa: E402

LDS_LIMIT = 160 * 1024
DYN_LDS = (2 * 8 * 8 * 256 + 4096) * 4          # mlp_launch: two unit buffers + the bias region


@pytest.fixture(scope='module')
def obj():
    from sda_amd import build as b
    b.build()                                            # incremental: a no-op when the objects are current
    return os.path.join(ROOT, 'sda_amd', 'lib', 'mlp1d.o')


def test_two_fragment_window_kernels_no_spills_no_scratch_lds_budget(obj):
    md = G.kernel_metadata(obj)
    dis = G.disassemble(obj)
    names = sorted(n for n in md if 'mlp_win2_' in n)
    # {forward, VJP} x {narrow, wide}, window mode only
    assert len(names) == 4 and sum('_wide' in n for n in names) == 2 and all('ILb1E' in n for n in names), names
    for n in names:
        k, ins = md[n], dis[n]
        assert k['vgpr_spill_count'] == 0, (n, k)
        assert not [i for i in ins if 'scratch_' in i], n
        assert k['group_segment_fixed_size'] + DYN_LDS <= LDS_LIMIT, (n, k)
        assert k['vgpr_count'] <= 512, (n, k)
        assert sum(1 for i in ins if 'v_mfma_f32_16x16x4' in i) > 0, n


def test_two_fragment_kernels_multiply_as_much_as_the_one_fragment_ones(obj):
    """The second fragment costs loader, epilogue and store instructions, no multiply: the MFMA counts are those of the one-fragment window
    kernels (the last GEMM of a window above 16 values is a 128-feature slab, as for every width above 16)."""
    dis = G.disassemble(obj)

    def mfmas(key):
        names = [n for n in dis if key in n]
        assert len(names) == 1, (key, names)
        return sum(1 for i in dis[names[0]] if 'v_mfma_f32_16x16x4' in i)
    for two, one in (('mlp_win2_fwdILb1E', 'mlp_fwd_kernelILb1E'), ('mlp_win2_bwdILb1E', 'mlp_bwd_kernelILb1E'),
                     ('mlp_win2_fwd_wideILb1E', 'mlp_fwd_kernel_wideILb1E'), ('mlp_win2_bwd_wideILb1E', 'mlp_bwd_kernel_wideILb1E')):
        assert mfmas(two) == mfmas(one), (two, one)
