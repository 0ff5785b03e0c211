"""Layer cases of the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip), shared by its host replay (test_wgrad3_host.py)
and its device tests (test_gpu_wgrad3.py).  Built by tests/wgrad_ref.py: the float64 reference is that module's.

Every case carries, beside its shape, the plan its author expects of the kernel's planner: rows per stage R, row
blocks per image nrb, the cout tile 32 mt, the tile counts n_ct / n_cit, the slab count and whether R (W + 2) is no multiple of
the four positions of a K step (``q4_rounds``: the last K step then reads the zeroed tail of the cotangent tile).  ``plan``
(tests/wgrad3_plan.py) works the same plan out in plain Python; the host test holds the table, ``plan`` and the library against one
another."""
from tests.wgrad3_plan import LDS_MAX, S1, pitch, plan as _plan  # noqa: F401
from tests.wgrad_ref import make_case

ACTS = ('ReLU', 'ELU', 'GELU', 'SELU')


def _case(kind, cin, cout, n, h, w, circular, seed, *, R, nrb, mt, n_ct, n_cit, slabs, q4_rounds, act=None):
    cfg = dict(kind=kind, cin=cin, cout=cout, n=n, h=h, w=w, circular=circular, seed=seed)
    if act is not None:
        cfg['act'] = act
    return dict(cfg=cfg, plan=dict(R=R, nrb=nrb, mt=mt, n_ct=n_ct, n_cit=n_cit, slabs=slabs, q4_rounds=q4_rounds))


_P1 = dict(mt=1, n_ct=1, n_cit=1)           # one 32 x 32 tile

_TABLE = {
    # the smallest shapes that reach every branch of the kernel:
    #   wrap      one cin tile, one 32-cout tile, wrap-around in both axes, plain loader, db present
    #   zero_act  W no power of two, H one ragged-free row block, two cin tiles, the 96-cout tile, border zeros, SiLU loader (conv2)
    #   ln_mod    the conv1 loader (LayerNorm statistics + a per-image modulation row: mod_sn != 0), three cin tiles, the 64-cout tile,
    #             W narrower than the four positions of a K step
    'wrap': _case('plain', 32, 32, 2, 8, 8, True, 41, R=8, nrb=1, slabs=2, q4_rounds=False, **_P1),
    'zero_act': _case('conv2', 64, 96, 3, 6, 10, False, 42, act='SiLU', R=6, nrb=1, mt=3, n_ct=1, n_cit=2, slabs=3, q4_rounds=False),
    'ln_mod': _case('conv1', 96, 64, 2, 16, 4, True, 43, R=16, nrb=1, mt=2, n_ct=1, n_cit=3, slabs=2, q4_rounds=False),
    # n_ct off 1 at the 96-cout tile; two cin tiles, so that a swapped ct / cit decode cannot cancel
    'ct_mt3': _case('plain', 64, 192, 1, 4, 4, True, 51, R=4, nrb=1, mt=3, n_ct=2, n_cit=2, slabs=1, q4_rounds=False),
    # n_ct off 1 at the 64-cout tile
    'ct_mt2': _case('conv2', 64, 128, 2, 4, 4, False, 52, act='SiLU', R=4, nrb=1, mt=2, n_ct=2, n_cit=2, slabs=2, q4_rounds=False),
    # n_ct = 5 at the 32-cout tile (160 is a multiple of neither 96 nor 64)
    'ct_mt1': _case('conv1', 32, 160, 1, 4, 4, True, 53, R=4, nrb=1, mt=1, n_ct=5, n_cit=1, slabs=1, q4_rounds=False),
    # R off H: one output row per stage (W + 2 > 64), three staged rows with a fresh halo every stage, nrb = H
    'row1': _case('conv2', 32, 32, 1, 3, 64, True, 54, act='SiLU', R=1, nrb=3, slabs=3, q4_rounds=True, **_P1),
    # ... and its halo rows as border zeros
    'row1_zero': _case('conv2', 32, 32, 1, 3, 64, False, 55, act='SiLU', R=1, nrb=3, slabs=3, q4_rounds=True, **_P1),
    # the widest W with two rows per stage (W + 2 = 64) ...
    'r_edge_62': _case('plain', 32, 32, 1, 2, 62, True, 56, R=2, nrb=1, slabs=1, q4_rounds=False, **_P1),
    # ... and the narrowest with one (W + 2 = 65)
    'r_edge_63': _case('plain', 32, 32, 1, 2, 63, True, 57, R=1, nrb=2, slabs=2, q4_rounds=True, **_P1),
    # q4 off R (W + 2): 21 positions in a K extent of 24, LayerNorm loader
    'q4_tail': _case('conv1', 32, 32, 2, 3, 5, True, 58, R=3, nrb=1, slabs=2, q4_rounds=True, **_P1),
    # ... with border zeros
    'q4_tail_zero': _case('conv1', 32, 32, 2, 3, 5, False, 59, R=3, nrb=1, slabs=2, q4_rounds=True, **_P1),
    # ... and 25 positions in 28, more rows than columns
    'q4_tail_col': _case('plain', 32, 32, 1, 5, 3, True, 60, R=5, nrb=1, slabs=1, q4_rounds=True, **_P1),
    # H = W = 1: every tap wraps onto the one pixel
    'one_pixel': _case('plain', 32, 32, 1, 1, 1, True, 61, R=1, nrb=1, slabs=1, q4_rounds=True, **_P1),
    # ... every tap but the centre is padding
    'one_pixel_zero': _case('plain', 32, 32, 1, 1, 1, False, 62, R=1, nrb=1, slabs=1, q4_rounds=True, **_P1),
    # mod_sn off cin: the conv1 loader with one modulation row shared by the images
    'shared_row': _case('conv1_shared', 32, 32, 2, 4, 4, True, 63, R=4, nrb=1, slabs=2, q4_rounds=False, **_P1),
    # per off 1 by the planner's own choice: 3 tiles -> s = 170 of S = 300 stages -> 2 stages per slab, 150 slabs
    'planner_per2': _case('plain', 96, 32, 300, 2, 2, True, 64, R=2, nrb=1, mt=1, n_ct=1, n_cit=3, slabs=150, q4_rounds=False),
    # the 192-channel level's W + 2 = 34 and R = 3 with a ragged last row block (2 live rows of 3), 24 stages
    'ragged_workload': _case('conv2', 32, 32, 2, 35, 32, False, 65, act='SiLU', R=3, nrb=12, slabs=24, q4_rounds=True, **_P1),
}
# act_in off SiLU: the other four activations of the conv2 loader
for _i, _act in enumerate(ACTS):
    _TABLE['act_' + _act] = _case('conv2', 32, 32, 1, 2, 2, True, 70 + _i, act=_act, R=2, nrb=1, slabs=1, q4_rounds=False, **_P1)

CASES = {name: entry['cfg'] for name, entry in _TABLE.items()}
PLANS = {name: entry['plan'] for name, entry in _TABLE.items()}

#: cout tile -> the largest W the kernel serves (cin 32, n = 1, h = 2: one row per stage): the 160 KiB LDS cap of the plan
BOUNDARY = {32: 306, 64: 242, 96: 190}
_BOUNDARY_KIND = {32: ('plain', True), 64: ('conv1', True), 96: ('conv2', False)}


def build(name, dev):
    cfg = dict(CASES[name])
    return make_case(cfg.pop('kind'), dev, **cfg)


def boundary_case(cout, dev, over=0):
    """The widest served layer of cout tile ``cout`` (``over`` = 1: the first one past it)."""
    kind, circular = _BOUNDARY_KIND[cout]
    return make_case(kind, dev, cin=32, cout=cout, n=1, h=2, w=BOUNDARY[cout] + over, circular=circular, seed=90 + cout // 32 + 4 * over)


def plan(cin, cout, n, h, w, slabs=0):
    """tests.wgrad3_plan.plan at the stride-1 geometry."""
    return _plan(S1, cin, cout, n, h, w, slabs)
