"""Which instance of csrc/conv_small1d.hip a launch reaches, and the launches tests/test_gpu_small1d.py runs.

`plan()` restates small1d_plan from the launch's n and wo (tests/test_small1d_host.py holds every case of this file against the
library's own answer, sda_small1d_tile, so the table cannot drift from the planner):

    16 positions per workgroup while n * ceil(wo / 16) <= TP_GRID, else 32 while n * ceil(wo / 32) <= TP_GRID, else 64;
    refused (0: the general kernels serve the launch) once n * ceil(wo / tile) > MAX_GRID.

A case is a dict:
  family     t64_multi | t64_short | t32 | t16_edge | t64_cap | cross        (the tolerance table of the GPU module is per family)
  tile       the tile the planner must give: 16 / 32 / 64, or 0 for the one launch the kernel declines
  n, wo      images, positions (wo == ws: k = 3, stride 1)
  cin, cout  of the LAUNCH: for transpose=True the layer is a Conv1d(cout -> cin) and the launch its backward-data form
  circular   padding
  fuse       a key of FUSIONS
  view       planar | channel_last | window | split     (how the source is laid out, see VIEWS)
  pack       own: PackedConv's padding (cin_pad % 8 == 0, cout_pad % 32 == 0) | tight: the narrowest the kernel takes
             (cin_pad % 4 == 0, cout_pad % 16 == 0)
  transpose  the weights are the backward-data packing of the layer
  chunks     view == 'split' only: ((first image, images, tile), ...) -- the launches whose outputs together must equal, bit for
             bit, the one launch over all n images
"""

TP_GRID = 1024
MAX_GRID = 4096
MAXC = 64

# what each fusion switches on: mod none | shared (one row, mod_sn = 0) | image (a row per image, mod_sn = cin); ln: LayerNorm with
# given statistics; act: the loader's activation; bias; dact: the epilogue's x act'(z); res: the residual add
_OFF = dict(mod='none', ln=False, act='none', bias=False, dact='none', res=False)
FUSIONS = {
    'off': dict(_OFF),
    'mod_shared': dict(_OFF, mod='shared'),
    'mod_image': dict(_OFF, mod='image'),
    'ln': dict(_OFF, ln=True),
    'act_silu': dict(_OFF, act='SiLU'),
    'act_elu': dict(_OFF, act='ELU'),
    'bias': dict(_OFF, bias=True),
    'dact_silu': dict(_OFF, dact='SiLU'),
    'dact_elu': dict(_OFF, dact='ELU'),
    'res': dict(_OFF, res=True),
    'all': dict(mod='shared', ln=True, act='SiLU', bias=True, dact='SiLU', res=True),
    # every out-of-line branch at once: per-image modulation, the rolled activation loop, the noinline act'
    'all_image_elu': dict(mod='image', ln=True, act='ELU', bias=True, dact='ELU', res=True),
    # all but the LayerNorm: for 3-channel sources, where a LayerNorm over nearly equal channels is ill-conditioned for every evaluator
    'all_but_ln': dict(mod='shared', ln=False, act='SiLU', bias=True, dact='SiLU', res=True),
}
EACH_FUSION = ('off', 'mod_shared', 'mod_image', 'ln', 'act_silu', 'act_elu', 'bias', 'dact_silu', 'dact_elu', 'res', 'all')

# window view: the source is a trajectory [B][L][C][ws]; image (b, i) takes the WINDOW consecutive time steps from i on as its
# WINDOW * C channels (n_inner = L - WINDOW + 1 windows per trajectory)
WINDOW = 5
VIEWS = ('planar', 'channel_last', 'window', 'split')


def ceil_div(a, b):
    return (a + b - 1) // b


def plan(n, wo, forced=0):
    """The tile small1d_plan gives an eligible launch of n images x wo positions (forced: SDA_SMALL1D_TP), 0 where it declines."""
    tile = 16 if n * ceil_div(wo, 16) <= TP_GRID else 32 if n * ceil_div(wo, 32) <= TP_GRID else 64
    if forced in (16, 32, 64):
        tile = forced
    return 0 if n * ceil_div(wo, tile) > MAX_GRID else tile


def round_up(v, m):
    return ceil_div(v, m) * m


def own_mt(cout):
    """ops.pick_mt: the cout tile 32 * mt, mt in 1..4, that pads least (ties: 3, 4, 2, 1)."""
    best, best_pad = 1, None
    for mt in (3, 4, 2, 1):
        pad = round_up(cout, 32 * mt)
        if best_pad is None or pad < best_pad:
            best, best_pad = mt, pad
    return best


def pads(case):
    """(cin_pad, cout_pad) of the case's weight packing."""
    if case['pack'] == 'tight':
        return round_up(case['cin'], 4), round_up(case['cout'], 16)
    return round_up(case['cin'], 8), round_up(case['cout'], 32 * own_mt(case['cout']))


def window_geometry(case):
    """(B, L, C, windows per trajectory) of a window-view case."""
    assert case['cin'] % WINDOW == 0
    nw = next(k for k in (19, 16, 9) if case['n'] % k == 0)
    return case['n'] // nw, nw + WINDOW - 1, case['cin'] // WINDOW, nw


def source_fields(case, lo=0, n=None):
    """The descriptor's source fields (element strides into the case's source storage) for images [lo, lo + n)."""
    cin, ws = case['cin'], case['wo']
    n = case['n'] if n is None else n
    if case['view'] == 'channel_last':                       # storage [n][ws][cin]
        return dict(n=n, cx=cin, hs=1, ws=ws, x_sn_outer=ws * cin, x_sn_inner=0, n_inner=1, x_n_off=lo, x_sc=1, x_sy=ws * cin, x_sx=cin)
    if case['view'] == 'window':                             # storage [B][L][C][ws]
        _, L, C, nw = window_geometry(case)
        return dict(n=n, cx=cin, hs=1, ws=ws, x_sn_outer=L * C * ws, x_sn_inner=C * ws, n_inner=nw, x_n_off=lo, x_sc=ws, x_sy=ws, x_sx=1)
    return dict(n=n, cx=cin, hs=1, ws=ws, x_sn_outer=cin * ws, x_sn_inner=0, n_inner=1, x_n_off=lo, x_sc=ws, x_sy=ws, x_sx=1)


def source_numel(case):
    if case['view'] == 'window':
        B, L, C, _ = window_geometry(case)
        return B * L * C * case['wo']
    return case['n'] * case['cin'] * case['wo']


def launches(case):
    """((first image, images, tile), ...): the launches of a case -- one, or the chunks of a split case after the whole."""
    whole = ((0, case['n'], case['tile']),)
    return whole + tuple(case['chunks']) if case['view'] == 'split' else whole


def case_id(case):
    s = f"{case['family']}-n{case['n']}-wo{case['wo']}-c{case['cin']}x{case['cout']}-{'circular' if case['circular'] else 'zeros'}-{case['fuse']}"
    s += '' if case['view'] == 'planar' else '-' + case['view']
    s += '-tight' if case['pack'] == 'tight' else ''
    s += '-T' if case['transpose'] else ''
    return s


def _case(family, tile, n, wo, ch, padding, fuse='all', view='planar', pack='own', transpose=False, chunks=()):
    assert fuse in FUSIONS and view in VIEWS and padding in ('zeros', 'circular')
    return dict(family=family, tile=tile, n=n, wo=wo, cin=ch[0], cout=ch[1], circular=padding == 'circular', fuse=fuse, view=view,
                pack=pack, transpose=transpose, chunks=tuple(chunks))


def _build():
    Z, C = 'zeros', 'circular'
    cs = []
    # ---- t64_multi, 342 x 97: two 64-position tiles, the last with 33 positions (fragments nf = 2, 3 partly / wholly past the end)
    cs += [_case('t64_multi', 64, 342, 97, (64, 64), Z), _case('t64_multi', 64, 342, 97, (64, 64), C, 'off'),
           _case('t64_multi', 64, 342, 97, (17, 33), C), _case('t64_multi', 64, 342, 97, (17, 33), Z, 'all_image_elu', pack='tight'),
           _case('t64_multi', 64, 342, 97, (3, 64), C, 'all_but_ln'), _case('t64_multi', 64, 342, 97, (64, 1), Z, pack='tight'),
           _case('t64_multi', 64, 342, 97, (40, 16), C, 'all_image_elu')]
    # ---- t64_short, 1025 sequences shorter than the tile and than the halo; with one position both circular neighbours are the
    # position itself
    for wo, ch, pack in ((1, (17, 33), 'own'), (2, (64, 1), 'own'), (3, (3, 64), 'own'), (5, (40, 16), 'tight'), (16, (64, 64), 'own')):
        for padding in (C, Z):
            cs.append(_case('t64_short', 64, 1025, wo, ch, padding, 'all_but_ln' if ch[0] == 3 else 'all', pack=pack))
    cs += [_case('t64_short', 64, 1025, 1, (64, 64), C, 'off'), _case('t64_short', 64, 1025, 2, (17, 33), C, 'all_image_elu', pack='tight')]
    # ---- t32: 513 x 32 fills its tile, 600 x 20 leaves fragment nf = 1 with 4 positions
    cs += [_case('t32', 32, 513, 32, (64, 64), Z), _case('t32', 32, 513, 32, (17, 33), C, pack='tight'),
           _case('t32', 32, 513, 32, (3, 64), C, 'all_but_ln'), _case('t32', 32, 513, 32, (40, 16), Z, 'off'),
           _case('t32', 32, 600, 20, (64, 64), C), _case('t32', 32, 600, 20, (64, 1), Z),
           _case('t32', 32, 600, 20, (40, 16), C, 'all_image_elu', pack='tight'), _case('t32', 32, 600, 20, (17, 33), Z, 'off')]
    # ---- t16_edge, 512 x 32: n * ceil(wo / 16) is exactly 1024
    cs += [_case('t16_edge', 16, 512, 32, (64, 64), C), _case('t16_edge', 16, 512, 32, (17, 33), Z, 'all_image_elu', pack='tight'),
           _case('t16_edge', 16, 512, 32, (3, 64), Z, 'all_but_ln'), _case('t16_edge', 16, 512, 32, (64, 1), C, 'off'),
           _case('t16_edge', 16, 512, 32, (40, 16), Z)]
    # ---- t64_cap: the last grid the kernel serves and the first it leaves to the general kernels
    for padding in (Z, C):
        cs += [_case('t64_cap', 64, 4096, 64, (4, 8), padding), _case('t64_cap', 0, 4097, 64, (4, 8), padding)]
    # ---- fusions: all off, each alone, all on -- on one shape per tile
    for family, tile, n, wo, ch, padding in (('t64_multi', 64, 342, 97, (17, 33), Z), ('t32', 32, 600, 20, (40, 16), C),
                                             ('t16_edge', 16, 512, 32, (17, 33), C)):
        have = {case_id(c) for c in cs}
        for fuse in EACH_FUSION:
            c = _case(family, tile, n, wo, ch, padding, fuse)
            if case_id(c) not in have:
                cs.append(c)
    # ---- source views, one shape per tile; the chunks of a split case have their own tiles
    for family, tile, n, wo, padding in (('t64_multi', 64, 342, 97, C), ('t32', 32, 513, 32, Z), ('t16_edge', 16, 512, 32, C)):
        cs += [_case(family, tile, n, wo, (17, 33), padding, 'all_image_elu', view='channel_last'),
               _case(family, tile, n, wo, (40, 16), padding, 'all_image_elu', view='window')]
    cs += [_case('t64_short', 64, 2052, 5, (40, 16), C, 'all_image_elu', view='split', chunks=((0, 1027, 64), (1027, 1025, 64))),
           _case('t32', 64, 1030, 32, (17, 33), Z, 'all_image_elu', view='split', chunks=((0, 515, 32), (515, 515, 32))),
           _case('t16_edge', 32, 600, 20, (64, 64), C, 'all_image_elu', view='split', chunks=((0, 301, 16), (301, 299, 16)))]
    # ---- backward data: the transposed packing of a Conv1d(cout -> cin, 3), on each tile
    for family, tile, n, wo in (('t64_multi', 64, 342, 97), ('t32', 32, 600, 20), ('t16_edge', 16, 512, 32)):
        cs += [_case(family, tile, n, wo, (33, 17), C, 'off', transpose=True), _case(family, tile, n, wo, (64, 3), Z, 'dact_silu', transpose=True)]
    return cs


CASES = _build()
# the one shape of the cross-tile and cross-route checks (its natural tile is 16; child processes force the others)
CROSS = _case('cross', 16, 4, 130, (40, 40), 'circular', 'all')
