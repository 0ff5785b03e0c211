"""Layer cases of the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip), shared by its host replay (test_wgrad3_host.py)
and its device tests (test_gpu_wgrad3.py).  Built by tests/wgrad_ref.py: the float64 reference is that module's."""
from tests.wgrad_ref import make_case

#: the smallest shapes that reach every branch of the kernel:
#:   wrap      one cin tile, one 32-cout tile, wrap-around in both axes, plain loader, db present
#:   zero_act  W no power of two, H one ragged-free row block, two cin tiles, the 96-cout tile, border zeros, SiLU loader (conv2)
#:   ln_mod    the conv1 loader (LayerNorm statistics + a per-image modulation row: mod_sn != 0), three cin tiles, the 64-cout tile,
#:             W narrower than the four positions of a K step
CASES = {
    'wrap': dict(kind='plain', cin=32, cout=32, n=2, h=8, w=8, circular=True, seed=41),
    'zero_act': dict(kind='conv2', cin=64, cout=96, n=3, h=6, w=10, circular=False, act='SiLU', seed=42),
    'ln_mod': dict(kind='conv1', cin=96, cout=64, n=2, h=16, w=4, circular=True, seed=43),
}


def build(name, dev):
    cfg = dict(CASES[name])
    return make_case(cfg.pop('kind'), dev, **cfg)
