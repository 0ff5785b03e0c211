"""Which kernel of csrc/norm.hip a call reaches, restated from named constants, and the shapes that reach each instantiation at its tail.

`route()` restates sda_ln_stats / ln_bwd_launch (tests/test_norm_cases_host.py reads every constant and table row back from the
source text and the kernel names from the built object, so neither can drift).  Not restated: the 2^31-block refusals and the
SDA_LN_*_QUAD=0 switches (the misaligned cases reach the same kernels).

`CASES` is the list tests/test_gpu_norm.py runs.  Three shapes carry it:
  QUAD  (3, c, 1, 5468)  16404 pixels, 1367 quads per image (odd: wavefronts of 8 and of 4 quads straddle images), 4101 quads in all:
                         5 over for workgroups of 32, 16 and 8 quads; w % 4 == 0, so the pooled quad kernels take it (gh at 2 x 10936)
  ODD   (3, c, 1, 5469)  16407 pixels, hw % 4 == 1: register, split and thread-per-pixel kernels; npix * SPLIT % 256 != 0 for every SPLIT
  SMALL (3, c, 1, 1365)  4095 pixels: one below the backward threshold; npix % 4 == 3 leaves the last workgroup of four wavefronts partial
and QUAD again with one pointer a float off 16-byte alignment, which must fall back to the register / split kernels."""
import itertools

LN_THREADS = 256
LN_SMALL_PIXELS = 16384
LN_BWD_SMALL_PIXELS = 4096
LN_QUAD_CMIN = 48
LN_QUAD_CMAX = 384
LN_REG_C = 96
# cmax, stats <lanes per quad, channels per lane, cooperating wavefronts>, bwd <lanes, channels, POOL = 1>, bwd_up <lanes, channels, POOL = 2>
LN_QUAD = [
    (64, (8, 8, 1), (8, 8, 1), (8, 12, 2)),
    (96, (8, 12, 1), (8, 12, 1), (8, 12, 2)),
    (128, (8, 16, 1), (8, 16, 1), (16, 12, 2)),
    (192, (8, 24, 1), (8, 24, 1), (16, 12, 2)),
    (256, (8, 8, 4), (16, 16, 1), (16, 24, 2)),
    (384, (8, 12, 4), (16, 24, 1), (16, 24, 2)),
]
# ln_bwd_split_pick: c <= bound -> <lanes per pixel, channels per lane>; None: every wider width
LN_SPLIT = [(96, (4, 24)), (192, (8, 24)), (None, (8, 48))]
# sda_ln_stats: ln_stats_reg_kernel<SPLIT> for LN_REG_C / 2 < c <= SPLIT * LN_REG_C
LN_REG_SPLITS = (1, 2, 4)

MOD_FORMS = ('none', 'image', 'column', 'shared')


def _quad_row(c):
    return next(r for r in LN_QUAD if c <= r[0])


def route(entry, n, c, h, w, pool=(1, 1), aligned=True):
    """The kernel instantiation a call launches: entry 'stats' | 'bwd' | 'apply'; aligned: every pointer the quad path checks is 16-byte
    aligned.  ('stats_wave',) ('stats_quad', lanes, cpl, nw) ('stats_reg', split) ('stats_plain',) ('bwd_quad', lanes, cpl, pool)
    ('bwd_split', lanes, cpl, pool) ('bwd_plain', ph, pw) ('bwd_wave', ph, pw) ('apply',)."""
    hw, npix = h * w, n * h * w
    quad_width = LN_QUAD_CMIN < c <= LN_QUAD_CMAX
    if entry == 'apply':
        return ('apply',)
    if entry == 'stats':
        if npix < LN_SMALL_PIXELS:
            return ('stats_wave',)
        if hw % 4 == 0 and quad_width and aligned:
            return ('stats_quad',) + _quad_row(c)[1]
        if LN_REG_C // 2 < c <= LN_REG_SPLITS[-1] * LN_REG_C:
            return ('stats_reg', next(s for s in LN_REG_SPLITS if c <= s * LN_REG_C))
        return ('stats_plain',)
    assert entry == 'bwd' and tuple(pool) in ((1, 1), (1, 2), (2, 2))
    pool = tuple(pool)
    small = npix < LN_BWD_SMALL_PIXELS
    wide = pool != (1, 2) and quad_width
    if not small and wide and (hw % 4 == 0 if pool == (1, 1) else w % 4 == 0) and aligned:
        return ('bwd_quad',) + _quad_row(c)[2 if pool == (1, 1) else 3]
    if not small and wide:
        return ('bwd_split',) + next(t for b, t in LN_SPLIT if b is None or c <= b) + (pool[0],)
    return ('bwd_wave' if small else 'bwd_plain',) + pool


def routable():
    """Every instantiation route() can name, over all widths, pixel counts either side of both thresholds, hw % 4, pool and alignment;
    plus the one-thread kernel sda_ln_bwd_amax launches in front of every backward."""
    out = {('apply',), ('amax_zero',)}
    for c, (h, w), aligned in itertools.product(range(1, LN_QUAD_CMAX + 2), ((1, 4095), (1, 4096), (1, 4097), (1, 16384), (1, 16385)),
                                                (True, False)):
        out.add(route('stats', 1, c, h, w, (1, 1), aligned))
        for pool in ((1, 1), (1, 2), (2, 2)):
            out.add(route('bwd', 1, c, h, w, pool, aligned))
    return out


def kernel_name(r):
    """The (function name, template arguments) of an instantiation as the object file spells it."""
    base = {'stats_wave': 'ln_stats_wave_kernel', 'stats_quad': 'ln_stats_quad_kernel', 'stats_reg': 'ln_stats_reg_kernel',
            'stats_plain': 'ln_stats_kernel', 'bwd_quad': 'ln_bwd_quad_kernel', 'bwd_split': 'ln_bwd_split_kernel',
            'bwd_plain': 'ln_bwd_kernel', 'bwd_wave': 'ln_bwd_wave_kernel', 'apply': 'ln_apply_kernel', 'amax_zero': 'ln_amax_zero_kernel'}
    return base[r[0]], tuple(r[1:])


def family(r):
    """wave | quad | quad_nw4 | split (register and split kernels) | plain (thread per pixel)."""
    kind = r[0].split('_')[1]
    if r[0] == 'stats_quad' and r[3] > 1:
        return 'quad_nw4'
    return 'split' if kind == 'reg' else kind


def units_per_workgroup(r):
    """(units, per workgroup) granularity of a quad, register or split kernel's grid: quads, or lanes (pixels x SPLIT)."""
    if r[0] == 'stats_quad':
        return 'quad', (64 // r[1]) * (LN_THREADS // 64) // r[3]
    if r[0] == 'bwd_quad':
        return 'quad', (64 // r[1]) * (LN_THREADS // 64)
    if r[0] in ('stats_reg', 'bwd_split'):
        return 'lane', LN_THREADS
    return None, None


def tail(case):
    """Units in the last, partial workgroup (0: the case has no tail) for a case on a quad, register or split kernel."""
    r = case_route(case)
    what, per = units_per_workgroup(r)
    npix = case['n'] * case['h'] * case['w']
    if what == 'quad':
        return (npix // 4) % per
    if what == 'lane':
        return (npix * r[1]) % per
    return None


def straddles(case):
    """Does some wavefront of a quad case hold quads of two images?"""
    r = case_route(case)
    qw, qpi = 64 // r[1], case['h'] * case['w'] // 4
    return any((k * qpi) % qw for k in range(1, case['n']))


def case_route(case):
    return route(case['entry'], case['n'], case['c'], case['h'], case['w'], case['pool'], case['misaligned'] is None)


def case_id(case):
    r = case_route(case)
    s = '-'.join(str(v) for v in r) + f"-c{case['c']}-{case['mod']}-{'u' if case['unbiased'] else 'b'}"
    s += '-res' if case['res'] else ''
    s += '-offset' if case['cond'] == 'offset' else ''
    s += f"-mis_{case['misaligned']}" if case['misaligned'] else ''
    return s


QUAD, ODD, SMALL = (3, 1, 5468), (3, 1, 5469), (3, 1, 1365)
FORM_A = dict(mod='column', res=True, unbiased=True, cond='plain')        # the block LayerNorms of the U-Net
FORM_B = dict(mod='none', res=False, unbiased=False, cond='plain')       # the tail LayerNorms under LN_UNBIASED = False
FORM_S = dict(mod='shared', res=True, unbiased=True, cond='offset')       # one modulation row for the whole batch; 1000 + randn
FORM_I = dict(mod='image', res=True, unbiased=False, cond='offset')


def _case(entry, shape, c, form, pool=(1, 1), misaligned=None, **flags):
    n, h, w = shape
    d = dict(entry=entry, n=n, c=c, h=h, w=w, pool=pool, misaligned=misaligned, apply=False, amax=None)
    d.update(form)
    if entry == 'stats':
        d['res'] = False
    d.update(flags)
    return d


def _build():
    S, B = 'stats', 'bwd'
    cs = []
    # ---- statistics
    # wave-per-pixel: the 64-lane channel stride with a short, an exact (64 is swept elsewhere; 63 / 65 sit either side) and a ragged last step
    cs += [_case(S, SMALL, 1, FORM_B, apply=True), _case(S, SMALL, 2, FORM_A, apply=True), _case(S, SMALL, 63, FORM_S, apply=True),
           _case(S, SMALL, 65, FORM_I, apply=True), _case(S, SMALL, 200, FORM_A)]
    # quad layouts: the row's cmax and a ragged width inside it
    for full, ragged in ((64, 50), (96, 70), (128, 100), (192, 130), (256, 200), (384, 300)):
        cs += [_case(S, QUAD, full, FORM_A), _case(S, QUAD, ragged, FORM_B)]
    # 1000 + randn on EVERY statistics layout: a one-pass variance in any one of them is wrong there by two orders of magnitude
    cs += [_case(S, QUAD, 50, FORM_S), _case(S, QUAD, 70, FORM_S), _case(S, QUAD, 128, FORM_I), _case(S, QUAD, 192, FORM_I),
           _case(S, QUAD, 300, FORM_S), _case(S, QUAD, 256, FORM_I)]
    # register kernels, 1 / 2 / 4 lanes per pixel; the misaligned fall-back supplies the family's shared / image / offset forms
    for full, ragged in ((96, 70), (192, 130), (384, 300)):
        cs += [_case(S, ODD, full, FORM_A), _case(S, ODD, ragged, FORM_B)]
    cs += [_case(S, QUAD, 96, FORM_S, misaligned='x'), _case(S, ODD, 130, FORM_S), _case(S, QUAD, 200, FORM_I, misaligned='mean')]
    # thread per pixel
    cs += [_case(S, ODD, 385, FORM_A), _case(S, ODD, 40, FORM_B), _case(S, ODD, 40, FORM_S), _case(S, ODD, 385, FORM_I)]
    # ---- backward
    cs += [_case(B, SMALL, 1, FORM_B), _case(B, SMALL, 2, FORM_A), _case(B, SMALL, 63, FORM_S), _case(B, SMALL, 65, FORM_I),
           _case(B, SMALL, 200, FORM_A),
           _case(B, SMALL, 200, FORM_A, (1, 2)), _case(B, SMALL, 63, FORM_B, (1, 2)),
           _case(B, SMALL, 65, FORM_A, (2, 2)), _case(B, SMALL, 2, FORM_B, (2, 2))]
    for full, ragged in ((64, 50), (96, 70), (128, 100), (192, 130), (256, 200), (384, 300)):
        cs += [_case(B, QUAD, full, FORM_A, amax={96: 'lanes8', 256: 'lanes16'}.get(full)), _case(B, QUAD, ragged, FORM_B)]
    for full, ragged in ((96, 50), (192, 130), (384, 200)):
        cs += [_case(B, QUAD, full, FORM_A, (2, 2), amax='pooled' if full == 96 else None), _case(B, QUAD, ragged, FORM_B, (2, 2))]
    cs += [_case(B, QUAD, 70, FORM_S), _case(B, QUAD, 130, FORM_I, (2, 2))]
    for full, ragged in ((96, 70), (192, 130), (384, 300)):
        cs += [_case(B, ODD, full, FORM_A, amax='fallback' if full == 96 else None), _case(B, ODD, ragged, FORM_B)]
    for full, ragged in ((96, 50), (192, 130), (384, 200)):
        cs += [_case(B, ODD, full, FORM_A, (2, 2)), _case(B, ODD, ragged, FORM_B, (2, 2))]
    cs += [_case(B, QUAD, 96, FORM_S, misaligned='gx'), _case(B, QUAD, 200, FORM_I, (2, 2), misaligned='x'),
           _case(B, QUAD, 192, FORM_A, misaligned='mean')]
    # thread per pixel; 1 x 2 pooling has no other kernel, so it runs it at the widths the quad table serves too
    cs += [_case(B, ODD, 385, FORM_A), _case(B, ODD, 40, FORM_B), _case(B, ODD, 385, FORM_A, (2, 2)), _case(B, ODD, 40, FORM_B, (2, 2)),
           _case(B, ODD, 96, FORM_A, (1, 2)), _case(B, ODD, 70, FORM_B, (1, 2)), _case(B, ODD, 385, FORM_S), _case(B, ODD, 40, FORM_I, (2, 2))]
    return cs


CASES = _build()
