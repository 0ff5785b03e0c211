"""CPU: which kernel sda_step1d_prologue picks (sda_step1d_prologue_path: 1 staged, 0 unstaged, < 0 refused) at every boundary of its rule, and
the argument checks of sda_step1d_prologue and sda_pc_correct_keyed.  Every call here returns before anything is launched and no address
is ever read.

The rule (csrc/step1d.hip), with nin = 2 nf and every row padded by 4 floats in the staged copy:
    vecs  = 4 (hidden + e + cp + nf)                                              bytes of biases and frequencies
    lds   = vecs + 4 (hidden (nin + 4) + e (hidden + 4) + cp (e + 4))             bytes of the staged kernel
    quads = (hidden nin + e hidden + cp e) / 4                                    16-byte loads of the staged copy
    staged <=> nin, hidden, e powers of two, nin >= 8, w0 / w2 / (cp ? wp) 16-byte aligned, lds <= 140 KiB = 143 360, quads <= 8 x 1024
    unstaged otherwise, refused (-2) if vecs > 48 KiB;  nf > 64, hidden > 1024, e > 256: refused (-2)."""
import pytest

BADARG, UNSUPPORTED = -1, -2
STAGED, UNSTAGED = 1, 0
PTR = 1 << 20               # a non-null, 16-byte aligned address that is never dereferenced


@pytest.fixture(scope='module')
def lib():
    from sda_amd import _lib
    return _lib.load()


def _lds(nf, hidden, e, cp):
    return 4 * (hidden + e + cp + nf) + 4 * (hidden * (2 * nf + 4) + e * (hidden + 4) + cp * (e + 4))


def _quads(nf, hidden, e, cp):
    return (hidden * 2 * nf + e * hidden + cp * e) // 4


def _path(lib, nf, hidden, e, cp, w0=PTR, w2=PTR, wp=PTR):
    return lib.sda_step1d_prologue_path(nf, hidden, e, cp, w0, w2, wp)


def test_the_lds_bound_bites_at_cp_486_before_the_load_slots():
    """stock embedding: 4 x 790 + 4 x (256 x 36 + 32 x 260 + 486 x 36) = 143 288 <= 143 360 < 143 436 (one more row: + 4 x 37); 7 984 loads"""
    assert _lds(16, 256, 32, 486) == 143288 and _lds(16, 256, 32, 487) == 143436
    assert _quads(16, 256, 32, 487) < 8192


def test_stock_embedding_is_staged_up_to_486_projection_rows(lib):
    assert _path(lib, 16, 256, 32, 486) == STAGED
    assert _path(lib, 16, 256, 32, 487) == UNSTAGED


def test_every_load_slot_in_use_is_staged_and_one_more_row_is_not(lib):
    """(512 x 32 + 32 x 512) / 4 = 8192 = S1_STAGE_MAX x S1_THREADS exactly, in 142 016 bytes; a projection row adds 8 loads"""
    assert _quads(16, 512, 32, 0) == 8192 and _lds(16, 512, 32, 0) == 142016
    assert _quads(16, 512, 32, 1) == 8200 and _lds(16, 512, 32, 1) <= 140 * 1024
    assert _path(lib, 16, 512, 32, 0, wp=None) == STAGED
    assert _path(lib, 16, 512, 32, 1) == UNSTAGED


def test_eight_input_features_is_the_floor_of_the_staged_kernel(lib):
    assert _path(lib, 4, 8, 4, 3) == STAGED                # nin == 8
    assert _path(lib, 2, 8, 4, 3) == UNSTAGED              # nin == 4: a power of two and a multiple of 4, below the floor


def test_a_weight_matrix_off_by_one_float_is_unstaged(lib):
    assert _path(lib, 16, 256, 32, 192) == STAGED
    assert _path(lib, 16, 256, 32, 192, w0=PTR + 4) == UNSTAGED
    assert _path(lib, 16, 256, 32, 192, w2=PTR + 4) == UNSTAGED
    assert _path(lib, 16, 256, 32, 192, wp=PTR + 4) == UNSTAGED
    for off in (8, 12):
        assert _path(lib, 16, 256, 32, 192, wp=PTR + off) == UNSTAGED
    assert _path(lib, 16, 256, 32, 192, w0=PTR + 16, w2=PTR + 32, wp=PTR + 48) == STAGED


def test_without_a_projection_its_weight_address_does_not_count(lib):
    assert _path(lib, 16, 256, 32, 0, wp=None) == STAGED
    assert _path(lib, 16, 256, 32, 0, wp=PTR + 4) == STAGED


@pytest.mark.parametrize('shape', [(12, 256, 32, 8), (16, 100, 32, 8), (16, 256, 24, 8), (13, 100, 24, 7)])
def test_row_lengths_that_are_no_power_of_two_are_unstaged(lib, shape):
    assert _path(lib, *shape) == UNSTAGED


def test_the_maxima_are_served_unstaged_and_one_past_each_is_unsupported(lib):
    assert _path(lib, 64, 1024, 256, 33) == UNSTAGED
    assert _path(lib, 65, 256, 32, 8) == UNSUPPORTED
    assert _path(lib, 16, 1025, 32, 8) == UNSUPPORTED
    assert _path(lib, 16, 256, 257, 8) == UNSUPPORTED
    # the launcher returns the same code (before any launch)
    for nf, hidden, e in ((65, 256, 32), (16, 1025, 32), (16, 256, 257)):
        assert _launch(lib, nf=nf, hidden=hidden, e=e) == UNSUPPORTED


def test_bias_vectors_that_do_not_fit_48_kib_are_unsupported(lib):
    """unstaged: 4 (hidden + e + cp + nf) bytes of dynamic LDS; 16 + 256 + 32 + 11 984 = 12 288 floats = 48 KiB exactly"""
    assert _path(lib, 16, 256, 32, 11984) == UNSTAGED
    assert _path(lib, 16, 256, 32, 11985) == UNSUPPORTED
    assert _launch(lib, cp=11985) == UNSUPPORTED


def test_the_pick_refuses_what_the_launcher_refuses_first(lib):
    assert _path(lib, 16, 256, 32, 8, wp=None) == BADARG
    assert _path(lib, 16, 256, 32, 8, w0=None) == BADARG and _path(lib, 16, 256, 32, 8, w2=None) == BADARG
    for shape in ((0, 256, 32, 8), (16, 0, 32, 8), (16, 256, 0, 8), (16, 256, 32, -1)):
        assert _path(lib, *shape) == BADARG
    assert _path(lib, 65, 256, 32, 8, wp=None) == BADARG            # (a bad argument before an unsupported size: the launcher's order)


def _launch(lib, table=PTR, row_len=5, istep=PTR, t_dev=None, nt=2, alpha_kind=1, sigma_kind=0, nf=16, hidden=256, e=32, wp=PTR, cp=192,
            **ptrs):
    p = dict(freqs=PTR, w0=PTR, b0=PTR, w2=PTR, b2=PTR, bp=PTR, out_coef=PTR, out_step=PTR, mod=PTR)
    p.update(ptrs)
    return lib.sda_step1d_prologue(table, row_len, istep, t_dev, nt, alpha_kind, 1e-3, 1.5, sigma_kind, p['freqs'], nf, p['w0'], p['b0'], hidden,
                                   p['w2'], p['b2'], e, wp, p['bp'], cp, p['out_coef'], p['out_step'], p['mod'], None)


def test_prologue_bad_arguments_return_before_launch(lib):
    assert _launch(lib, wp=None) == BADARG                                             # cp > 0 without a projection matrix
    assert _launch(lib, nt=1) == BADARG and _launch(lib, nt=3) == BADARG              # a table row holds exactly two times
    assert _launch(lib, row_len=4) == BADARG
    assert _launch(lib, istep=None) == BADARG
    for nt in (0, 3):
        assert _launch(lib, table=None, istep=None, t_dev=PTR, nt=nt) == BADARG
    assert _launch(lib, table=None, istep=None, t_dev=None, nt=1) == BADARG
    for kind in (-1, 3):
        assert _launch(lib, alpha_kind=kind) == BADARG
        assert _launch(lib, sigma_kind=kind) == BADARG
    for name in ('freqs', 'w0', 'b0', 'w2', 'b2', 'out_coef', 'mod'):
        assert _launch(lib, **{name: None}) == BADARG, name
    # a bad argument wins over an unsupported size, whichever function finds it
    assert _launch(lib, nf=65, alpha_kind=3) == BADARG and _launch(lib, nf=65, wp=None) == BADARG


def test_pc_correct_keyed_bad_arguments_return_before_launch(lib):
    def call(x=PTR, eps=PTR, b=4, per=195, partial=PTR, nchunk=1, row0=0, draw_dev=PTR):
        return lib.sda_pc_correct_keyed(x, eps, b, per, partial, nchunk, 0.25, 0.0, PTR, 1234, row0, draw_dev, 1, 0, None)
    assert call(draw_dev=None) == BADARG
    assert call(b=65536) == BADARG
    assert call(row0=-1) == BADARG
    assert call(x=None) == BADARG and call(eps=None) == BADARG and call(partial=None) == BADARG
    assert call(b=0) == BADARG and call(per=0) == BADARG and call(nchunk=0) == BADARG


def test_abi_version_is_unchanged(lib):
    assert lib.sda_abi_version() == 14
