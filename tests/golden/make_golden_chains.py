#!/usr/bin/env python3 -B
"""Golden fixtures for the Markov chains and the particle-filter ground truth, generated FROM THE REFERENCE's sda/mcs.py and
experiments/lorenz/utils.py.

Runs only in the build container (needs /root/reference).  `sda/mcs.py` imports jax at module level and `sda/utils.py` imports
h5py and POT (`ot`); none of them is touched by the Lorenz / Lotka-Volterra chains, `bpf`, `log_prior`, `log_likelihood` or
`posterior`, so empty module objects are registered under those names purely so that the files can be executed.  The
fixture (tests/golden/chains.npz) holds arrays only.

Usage:  python3 -B tests/golden/make_golden_chains.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import make_golden as G  # noqa: E402  (zuko stand-in + reference loader)

#: fixture name -> (reference class name, constructor arguments); tests/test_chains_host.py builds the same chains
CHAINS = {
    'l63': ('Lorenz63', {}),
    'l63_s2': ('Lorenz63', {'dt': 0.025, 'steps': 2}),
    'l96_4': ('Lorenz96', {'n': 4}),
    'l96_5': ('Lorenz96', {'n': 5}),
    'l96_32': ('Lorenz96', {'n': 32}),
    'l96_40': ('Lorenz96', {'n': 40}),
    'l96_64': ('Lorenz96', {'n': 64}),
    'lv': ('LotkaVolterra', {}),
}


def _exec(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    G._load_reference()
    for name in ('jax', 'jax.numpy', 'jax.random', 'h5py', 'ot'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            if '.' in name:
                setattr(sys.modules[name.split('.')[0]], name.split('.')[1], sys.modules[name])
    mcs = _exec('sda.mcs', os.path.join(G.REF, 'sda', 'mcs.py'))
    _exec('sda.utils', os.path.join(G.REF, 'sda', 'utils.py'))
    cwd = os.getcwd()
    os.chdir(os.environ.get('TMPDIR', '/tmp'))                # the driver creates its PATH ('.') at import
    lor = _exec('ref_lorenz_utils', os.path.join(G.REF, 'experiments', 'lorenz', 'utils.py'))
    os.chdir(cwd)
    from oracle import sda_oracle as O

    out = {}
    torch.manual_seed(31)
    for key, (cls, kw) in CHAINS.items():
        chain = getattr(mcs, cls)(**kw)
        x0 = chain.prior((7,))
        out[f'{key}/x0'] = x0
        out[f'{key}/trans32'] = chain.transition(x0)
        out[f'{key}/traj32'] = chain.trajectory(x0, 16)
        out[f'{key}/trans64'] = chain.transition(x0.double())
        out[f'{key}/traj64'] = chain.trajectory(x0.double(), 16)

    # ---------------------------------------------------------------- preprocess / postprocess
    xs = mcs.Lorenz63().prior((7,))
    out['pre/x'] = xs
    out['pre/pre'] = mcs.Lorenz63.preprocess(xs)
    out['pre/post'] = mcs.Lorenz63.postprocess(mcs.Lorenz63.preprocess(xs))

    # ---------------------------------------------------------------- log_prob / log_prior / log_likelihood, 5 x (9, 3)
    torch.manual_seed(32)
    chain = lor.make_chain()
    x = chain.trajectory(chain.trajectory(chain.prior((5,)), 64, last=True), 9).transpose(0, 1).contiguous()       # (5, 9, 3)
    A = lambda v: chain.preprocess(v)[..., :1]      # noqa: E731
    y = torch.normal(A(x[:, ::2]), 0.25)
    out['lp/x'] = x
    out['lp/y'] = y
    for tag, cast in (('32', torch.float32), ('64', torch.float64)):
        xc, yc = x.to(cast), y.to(cast)
        out[f'lp/log_prob{tag}'] = chain.log_prob(xc[:, :-1], xc[:, 1:])
        out[f'lp/log_prior{tag}'] = lor.log_prior(xc)
        out[f'lp/log_lik{tag}'] = lor.log_likelihood(yc, xc, A=A, sigma=0.25, step=2)

    # ---------------------------------------------------------------- a small posterior problem: 4 observations, step 2
    torch.manual_seed(33)
    xt = chain.trajectory(chain.trajectory(chain.prior(()), 64, last=True), 7)             # (7, 3): times step .. 4 step
    yp = torch.normal(A(xt[::2]), 0.25)                                                    # (4, 1)
    out['post/x_true'] = xt
    out['post/y'] = yp
    runs = []
    for r in range(10):
        torch.manual_seed(100 + r)
        runs.append(lor.posterior(yp, A=A, sigma=0.25, step=2, particles=2048)[:256])
    out['post/A'], out['post/B'] = runs[0], runs[1]
    out['post/emd_ref'] = np.array([float(O.emd(runs[0], runs[2 + i])) for i in range(8)])
    out['post/emd_AB'] = np.array(float(O.emd(runs[0], runs[1])))
    G._save('chains', **out)


if __name__ == '__main__':
    main()
