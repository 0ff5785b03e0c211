"""Layer cases of the tiled weight-gradient kernel of the stride-2 heads and up-sampling tails (csrc/conv_wgrad3.hip), shared by its
host replay (test_wgrad3x_host.py) and its device tests (test_gpu_wgrad3x.py).  Built by tests/wgrad_ref.py ('tail_up', 'head_s2'):
the float64 reference is that module's.  ``h`` and ``w`` are the SOURCE size: the output is (2 h, 2 w) for 'tail_up' and
(h / 2, w / 2) for 'head_s2'.  'tail_up_plain' is 'tail_up' without the LayerNorm (the kernel's second up2 loader).

Every case carries, beside its shape, the plan its author expects of the kernel's planner: rows per stage R, row
blocks per image nrb, the cout tile 32 mt, the tile counts n_ct / n_cit, the slab count and whether R (wo + 2) is no multiple of
the four positions of a K step (``q4_rounds``).  ``plan`` (tests/wgrad3_plan.py) works the same plan out in plain Python; the
host test holds the table, ``plan`` and the library against one another."""
from tests.wgrad3_plan import LDS_MAX, S2, UP2, out_size, pitch, plan  # noqa: F401
from tests.wgrad_ref import make_case

UP2_PLAIN = 'tail_up_plain'


def _case(kind, cin, cout, n, h, w, circular, seed, *, R, nrb, mt, n_ct, n_cit, slabs, q4_rounds):
    cfg = dict(kind=kind, cin=cin, cout=cout, n=n, h=h, w=w, circular=circular, seed=seed)
    return dict(cfg=cfg, plan=dict(R=R, nrb=nrb, mt=mt, n_ct=n_ct, n_cit=n_cit, slabs=slabs, q4_rounds=q4_rounds))


_P1 = dict(mt=1, n_ct=1, n_cit=1)           # one 32 x 32 tile

_TABLE = {
    # one 32 x 32 tile, both geometries, both paddings (up2: 4 x 4 -> 8 x 8, W2 = 10; s2: 8 x 8 -> 4 x 4, W2 = 6)
    'up_wrap': _case(UP2, 32, 32, 2, 4, 4, True, 141, R=8, nrb=1, slabs=2, q4_rounds=False, **_P1),
    'up_zero': _case(UP2, 32, 32, 2, 4, 4, False, 142, R=8, nrb=1, slabs=2, q4_rounds=False, **_P1),
    's2_wrap': _case(S2, 32, 32, 2, 8, 8, True, 143, R=4, nrb=1, slabs=2, q4_rounds=False, **_P1),
    's2_zero': _case(S2, 32, 32, 2, 8, 8, False, 144, R=4, nrb=1, slabs=2, q4_rounds=False, **_P1),
    # the up2 kernel's other loader: no LayerNorm
    'up_plain': _case(UP2_PLAIN, 32, 32, 2, 3, 4, True, 145, R=6, nrb=1, slabs=2, q4_rounds=False, **_P1),
    'up_plain_zero': _case(UP2_PLAIN, 32, 32, 1, 2, 3, False, 146, R=4, nrb=1, slabs=1, q4_rounds=False, **_P1),
    # two cout tiles and two cin tiles at the 96-cout tile, non-square so that a swapped decode cannot cancel
    'up_ct_mt3': _case(UP2, 64, 192, 1, 2, 3, True, 151, R=4, nrb=1, mt=3, n_ct=2, n_cit=2, slabs=1, q4_rounds=False),
    's2_ct_mt3': _case(S2, 64, 192, 1, 4, 6, False, 152, R=2, nrb=1, mt=3, n_ct=2, n_cit=2, slabs=1, q4_rounds=True),
    # ... at the 64-cout tile
    'up_ct_mt2': _case(UP2, 64, 128, 2, 3, 2, False, 153, R=6, nrb=1, mt=2, n_ct=2, n_cit=2, slabs=2, q4_rounds=False),
    's2_ct_mt2': _case(S2, 64, 128, 2, 6, 4, True, 154, R=3, nrb=1, mt=2, n_ct=2, n_cit=2, slabs=2, q4_rounds=False),
    # ... at the 32-cout tile (160 is a multiple of neither 96 nor 64): n_ct = 5, with two and three cin tiles
    'up_ct_mt1': _case(UP2, 64, 160, 1, 2, 1, True, 155, R=4, nrb=1, mt=1, n_ct=5, n_cit=2, slabs=1, q4_rounds=False),
    's2_ct_mt1': _case(S2, 96, 160, 1, 2, 4, False, 156, R=1, nrb=1, mt=1, n_ct=5, n_cit=3, slabs=1, q4_rounds=False),
    # a ragged last row block: 14 output rows in blocks of 12 (W2 = 10), 2 live rows in the second
    'up_ragged': _case(UP2, 32, 32, 1, 7, 4, True, 157, R=12, nrb=2, slabs=2, q4_rounds=False, **_P1),
    'up_ragged_zero': _case(UP2, 32, 32, 1, 7, 4, False, 158, R=12, nrb=2, slabs=2, q4_rounds=False, **_P1),
    's2_ragged': _case(S2, 32, 32, 1, 28, 16, True, 159, R=12, nrb=2, slabs=2, q4_rounds=False, **_P1),
    's2_ragged_zero': _case(S2, 32, 32, 1, 28, 16, False, 160, R=12, nrb=2, slabs=2, q4_rounds=False, **_P1),
    # one output row per stage (wo + 2 = 66 > 64), a fresh halo every stage; the up2 one is the workload's pitch at wo = 64
    'up_row1': _case(UP2, 32, 32, 1, 2, 32, True, 161, R=1, nrb=4, slabs=4, q4_rounds=True, **_P1),
    'up_row1_zero': _case(UP2, 32, 32, 1, 2, 32, False, 162, R=1, nrb=4, slabs=4, q4_rounds=True, **_P1),
    's2_row1': _case(S2, 32, 32, 1, 4, 128, True, 163, R=1, nrb=2, slabs=2, q4_rounds=True, **_P1),
    's2_row1_zero': _case(S2, 32, 32, 1, 4, 128, False, 164, R=1, nrb=2, slabs=2, q4_rounds=True, **_P1),
    # a K extent that is no multiple of 4: up2 9 rows of 14 (126 in 128) with one live row in the second block; s2 3 rows of 5 (15 in 16)
    'up_q4_tail': _case(UP2, 32, 32, 2, 5, 6, False, 165, R=9, nrb=2, slabs=4, q4_rounds=True, **_P1),
    's2_q4_tail': _case(S2, 32, 32, 2, 6, 6, True, 166, R=3, nrb=1, slabs=2, q4_rounds=True, **_P1),
    's2_q4_tail_zero': _case(S2, 32, 32, 2, 6, 6, False, 167, R=3, nrb=1, slabs=2, q4_rounds=True, **_P1),
    # the one-pixel extremes: up2 source 1 x 1 (every tap reads the one pixel, or padding); s2 source 2 x 2 -> output 1 x 1
    'up_one_pixel': _case(UP2, 32, 32, 1, 1, 1, True, 168, R=2, nrb=1, slabs=1, q4_rounds=False, **_P1),
    'up_one_pixel_zero': _case(UP2, 32, 32, 1, 1, 1, False, 169, R=2, nrb=1, slabs=1, q4_rounds=False, **_P1),
    's2_one_pixel': _case(S2, 32, 32, 1, 2, 2, True, 170, R=1, nrb=1, slabs=1, q4_rounds=True, **_P1),
    's2_one_pixel_zero': _case(S2, 32, 32, 1, 2, 2, False, 171, R=1, nrb=1, slabs=1, q4_rounds=True, **_P1),
    # per off 1 by the planner's own choice: 3 tiles -> s = 170 of S = 300 stages -> 2 stages per slab, 150 slabs
    'up_planner_per2': _case(UP2, 96, 32, 300, 1, 1, True, 172, R=2, nrb=1, mt=1, n_ct=1, n_cit=3, slabs=150, q4_rounds=False),
    's2_planner_per2': _case(S2, 96, 32, 300, 2, 2, False, 173, R=1, nrb=1, mt=1, n_ct=1, n_cit=3, slabs=150, q4_rounds=True),
    # the workload's row pitches: wo = 32 (W2 = 34, R = 3, ragged: 2 live rows in the 11th block) and wo = 16 (W2 = 18, R = 7, ragged)
    'up_workload_32': _case(UP2, 32, 32, 1, 16, 16, True, 174, R=3, nrb=11, slabs=11, q4_rounds=True, **_P1),
    's2_workload_32': _case(S2, 32, 32, 1, 64, 64, True, 175, R=3, nrb=11, slabs=11, q4_rounds=True, **_P1),
    'up_workload_16': _case(UP2, 32, 32, 1, 8, 8, False, 176, R=7, nrb=3, slabs=3, q4_rounds=True, **_P1),
    's2_workload_16': _case(S2, 32, 32, 1, 32, 32, True, 177, R=7, nrb=3, slabs=3, q4_rounds=True, **_P1),
}

CASES = {name: entry['cfg'] for name, entry in _TABLE.items()}
PLANS = {name: entry['plan'] for name, entry in _TABLE.items()}

#: (geometry, cout tile) -> the largest SOURCE width the kernel serves at one row per stage (cin 32, n = 1; source height 1 for
#: up2, 2 for s2), from the LDS formula of ``plan`` (test_wgrad3x_host.test_lds_cap_by_hand works them out again):
#:   up2, wo = 2 w: 4 (32 pitch(q4 + 2 (wo + 2) + 2) + 32 mt pitch(q4)), q4 = wo + 2 rounded up to 4 -> wo = 306 / 242 / 190
#:   s2,  wo = w / 2: 4 (32 pitch(7 (wo + 2) + q4 + 1) + 32 mt pitch(q4)) -> wo = 134 / 122 / 106; one past is the next EVEN width
BOUNDARY = {(UP2, 32): 153, (UP2, 64): 121, (UP2, 96): 95, (S2, 32): 268, (S2, 64): 244, (S2, 96): 212}
_BOUNDARY_H = {UP2: 1, S2: 2}
_BOUNDARY_STEP = {UP2: 1, S2: 2}


def build(name, dev):
    cfg = dict(CASES[name])
    return make(cfg.pop('kind'), dev, **cfg)


def make(kind, dev, **cfg):
    """tests.wgrad_ref.make_case, and 'tail_up_plain': the up-sampling tail read without its LayerNorm."""
    if kind != UP2_PLAIN:
        return make_case(kind, dev, **cfg)
    case = make_case(UP2, dev, **cfg)
    case['conv'].ln_mean = case['conv'].ln_rstd = None
    a = case['keep'][0].detach().double().cpu()
    case['v64'] = a.repeat_interleave(2, dim=3).repeat_interleave(2, dim=2)
    return case


def boundary_case(kind, cout, dev, over=0):
    """The widest served layer of geometry ``kind`` and cout tile ``cout`` (``over`` = 1: the first one past it)."""
    w = BOUNDARY[(kind, cout)] + over * _BOUNDARY_STEP[kind]
    return make_case(kind, dev, cin=32, cout=cout, n=1, h=_BOUNDARY_H[kind], w=w, circular=cout != 64,
                     seed=190 + cout // 32 + 4 * over + (8 if kind == S2 else 0))
