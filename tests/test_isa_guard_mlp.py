"""CPU build-time guard for the whole-MLP kernels (csrc/mlp1d.hip), in the manner of tests/test_isa_guard.py: the wide kernels hold a
wave's 16 rows x 256 features three times over next to the A fragments -- they fit the 512 registers of a wave at one wave per SIMD only
while the compiler spills nothing; a scratch access in those kernels sits in the vector-memory queue the slab staging counts on."""
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


def test_mlp_kernels_no_spills_no_scratch_lds_budget(obj):
    md = G.kernel_metadata(obj)
    dis = G.disassemble(obj)
    names = sorted(n for n in md if 'mlp_fwd_kernel' in n or 'mlp_bwd_kernel' in n)
    # {forward, VJP} x {rows, windows} x {narrow, wide}
    assert len(names) == 8 and sum('_wide' in n for n in names) == 4, names
    for n in names:
        k, ins = md[n], dis[n]
        assert k['vgpr_spill_count'] == 0, (n, k)
        assert not [i for i in ins if 'scratch_' in i], n
        assert k['group_segment_fixed_size'] + DYN_LDS <= LDS_LIMIT, (n, k)
        assert k['vgpr_count'] <= 512, (n, k)
        assert sum(1 for i in ins if 'v_mfma_f32_16x16x4' in i) > 0, n


# instructions / MFMAs of the eight kernels as the compiler emits them: the totals of commit 3b73fbe, whose narrow kernels held inline copies of
# the helpers they now call (ml_ln, ml_ln_bwd, ml_win_fold) -- the same opcodes in the same order, registers renamed
NARROW = {'mlp_fwd_kernelILb0E': (10000, 1404), 'mlp_fwd_kernelILb1E': (11090, 1404),
          'mlp_bwd_kernelILb0E': (8711, 936), 'mlp_bwd_kernelILb1E': (8321, 936)}
WIDE = {'mlp_fwd_kernel_wideILb0E': (17377, 1428), 'mlp_fwd_kernel_wideILb1E': (18188, 1428),
        'mlp_bwd_kernel_wideILb0E': (16300, 1428), 'mlp_bwd_kernel_wideILb1E': (14797, 1428)}


def _pinned(dis, pins):
    for key, (n_ins, n_mfma) in pins.items():
        names = [n for n in dis if key in n]
        assert len(names) == 1, (key, names)
        ins = dis[names[0]]
        assert (len(ins), sum(1 for i in ins if 'v_mfma_f32_16x16x4' in i)) == (n_ins, n_mfma), names[0]


def test_narrow_kernels_are_the_code_they_were(obj):
    """Nets whose GEMMs are all <= 128 wide must run what they ran before the wide kernels existed.  The narrow and the wide kernels share a
    translation unit and their helpers (ml_mm, ml_ln / ml_ln_bwd, ml_win_fold, ml_load_rows / ml_store_rows as templates): the narrow kernels'
    instruction and MFMA counts are pinned here.  The full comparison is `llvm-objdump -d --no-show-raw-insn` of the gfx950 code object of
    mlp1d.o (tools/isa_guard.py: disassemble) of this build against the previous one, kernel by kernel: equal lists.  A deliberate change to the
    narrow kernels, or a compiler update, moves these numbers -- then re-measure `tools/mlp_bench.py` and `bench.py --workload lorenz_eval
    --lorenz-net local` against the previous build, both libraries alternating in one session, and re-pin."""
    _pinned(G.disassemble(obj), NARROW)


def test_wide_kernels_are_the_code_they_were(obj):
    """The same pin for the four _wide kernels: they share every helper with the narrow ones, so an edit of a helper that disturbs them shows here."""
    _pinned(G.disassemble(obj), WIDE)
