#!/usr/bin/env python3
"""Time ONE analysis of the domain-localised smoother (csrc/enks_local.hip: prepare, pack, per-block weights, transform) over a
9-slab window against the same arithmetic in torch ops on the same device: the per-block [G | B] as batched float64 products over
the padded lists, a batched float64 ``cholesky_solve`` over the blocks, then a batched matmul over the blocks' components.  The
observed values H = Coarsen(4)(members) are taken once, outside the timing: what is timed is the analysis.

Cases (M, grid, block, radius): (64, 2 x 64 x 64, 4 x 4, 8) and (64, 2 x 256 x 256, 8 x 8, 16).  The routes alternate inside one
process: a block times CALLS calls of one route, then of the other; reported are the median of 5 blocks (per call) with the
fastest and the slowest block, after one warm-up block.  No speed is promised: where the kernels are slower the result says so.

    python tools/enks_local_bench.py [--out profiles/enks_local_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import observe, ops  # noqa: E402

CALLS, BLOCKS, SLABS = 10, 5, 9
SHAPES = [('M64_2x64x64_b4x4_r8', 64, (2, 64, 64), (4, 4), 8.0), ('M64_2x256x256_b8x8_r16', 64, (2, 256, 256), (8, 8), 16.0)]


def torch_tables(plan, dev):
    """The plan as padded (nblk, nmax) index / weight tables (weight 0 on the padding) and the (nblk, nb) component indices."""
    off = torch.from_numpy(plan.offsets_host.astype('int64'))
    n = off[1:] - off[:-1]
    nmax = int(n.max())
    idx = torch.zeros(plan.nblk, nmax, dtype=torch.int64)
    rho = torch.zeros(plan.nblk, nmax, dtype=torch.float64)
    mask = torch.arange(nmax)[None] < n[:, None]
    idx[mask] = torch.from_numpy(plan.idx_host.astype('int64'))
    rho[mask] = torch.from_numpy(plan.rho_host.astype('float64'))
    C, Hg, Wg = plan.event
    bh, bw = plan.block
    comp = torch.arange(C * Hg * Wg).reshape(C, Hg // bh, bh, Wg // bw, bw).permute(1, 3, 0, 2, 4).reshape(plan.nblk, -1)
    return idx.to(dev), rho.to(dev), comp.to(dev)


def torch_analysis(S, H, y, sigma, eps, idx, rho, comp):
    m = H.shape[0]
    Y = H - H.double().mean(dim=0).float()
    D = (y + sigma * eps) - H
    Yb = Y.double().T[idx]                                             # (nblk, nmax, m)
    Db = D.double().T[idx]
    Yw = Yb * rho[..., None]
    G = Yw.transpose(1, 2) @ Yb / (m - 1) + sigma ** 2 * torch.eye(m, device=H.device, dtype=torch.float64)
    W = torch.cholesky_solve(Yw.transpose(1, 2) @ Db / (m - 1), torch.linalg.cholesky(G)).float()      # (nblk, m, m)
    X = S[:, :, comp]                                                  # (slabs, m, nblk, nb)
    X = X + torch.einsum('bmj,smbq->sjbq', W, X - X.mean(dim=1, keepdim=True))
    S[:, :, comp] = X
    return S


def block(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def stats(ts):
    return {'median': round(statistics.median(ts), 4), 'fastest': round(min(ts), 4), 'slowest': round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/enks_local_bench.json')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    sigma = 0.5
    result = {'device': torch.cuda.get_device_name(0), 'calls_per_block': CALLS, 'blocks': BLOCKS, 'slabs': SLABS, 'sigma': sigma,
              'operator': 'Coarsen(4)', 'unit': 'ms per analysis', 'cases': {}}
    A = observe.Coarsen(4)
    for name, m, event, blk, radius in SHAPES:
        torch.manual_seed(0)
        d = event[0] * event[1] * event[2]
        S0 = torch.randn(SLABS, m, d, device=dev) + torch.randn(1, m, d, device=dev)
        H = A(S0[-1].reshape(m, *event)).reshape(m, -1).contiguous()
        k = H.shape[1]
        plan = ops.enkl_plan(event, observe.positions(A, event), radius, blk, device=dev)
        idx, rho, comp = torch_tables(plan, dev)
        y = H.mean(dim=0) + 0.3 * torch.randn(k, device=dev)
        eps = torch.randn(m, k, device=dev)
        S = S0.clone()
        Y, D, E = (torch.empty(m, k, device=dev) for _ in range(3))
        W = torch.empty(plan.nblk, m, m, device=dev)
        status = torch.zeros(plan.nblk, device=dev, dtype=torch.int32)

        def device():
            ops.enkw_prepare(H, y, sigma, seed=1, draw=0, Y=Y, D=D, eps=E)
            ops.enkl_weights(plan, Y, D, sigma, W=W, status=status)
            ops.enkl_transform(plan, S, 0, SLABS - 1, W)

        routes = {'device': device, 'torch': lambda: torch_analysis(S, H, y, sigma, eps, idx, rho, comp)}
        times = {r: [] for r in routes}
        for r, fn in routes.items():                      # warm-up; every route starts a block from the same ensemble
            S.copy_(S0)
            block(fn)
        for _ in range(BLOCKS):
            for r, fn in routes.items():
                S.copy_(S0)
                times[r].append(block(fn))
        res = {'members': m, 'grid': list(event), 'block': list(blk), 'radius': radius, 'k': k, 'nblk': plan.nblk,
               'longest_list': int((plan.offsets_host[1:] - plan.offsets_host[:-1]).max()),
               **{r + '_ms': stats(ts) for r, ts in times.items()}}
        res['device_median_below_torch_fastest'] = res['device_ms']['median'] < res['torch_ms']['fastest']
        result['cases'][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
