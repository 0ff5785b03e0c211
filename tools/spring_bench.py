"""Time the exact linear-Gaussian routes (csrc/lgss.hip) against the same recursions written with torch ops on the device.

    python tools/spring_bench.py            # writes profiles/lgss_bench.json

posterior: 16 384 samples at (N = 65, step = 1) and (N = 9, step = 8), device route (tables on the host, one filter launch, one sampler
launch) against a torch-ops forward filter / backward sampler in float64 on the device.  ExactScore: batch 1024, length 65, against a
dense float64 torch.linalg.solve on the device.  The routes alternate inside one process; per route the median of 5 blocks with the
fastest and the slowest block kept.  As information: emd and mean error of the generic bootstrap filter (sda_amd.utils.bpf, 16 384
particles) against the exact posterior."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sda_amd import metrics, ops  # noqa: E402
from sda_amd.experiments import spring  # noqa: E402

DEV = torch.device('cuda')
BLOCKS, REPS = 5, 3
OBS = lambda x: x[..., :1]  # noqa: E731


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


def alternate(routes):
    """{name: callable} -> {name: {median_ms, fastest_ms, slowest_ms}}, the routes taking turns block by block."""
    for fn in routes.values():
        fn()                                                        # warm-up
    times = {k: [] for k in routes}
    for _ in range(BLOCKS):
        for k, fn in routes.items():
            times[k].append(timed(fn))
    return {k: dict(median_ms=statistics.median(v), fastest_ms=min(v), slowest_ms=max(v)) for k, v in times.items()}


def torch_posterior(y, sigma, step, samples, burn=64):
    """The same forward filter / backward sampler in torch ops (float64 on the device, torch's generator for the normals)."""
    chain = spring.make_chain()
    A, b, Q = (v.double().to(DEV) for v in (chain.A, chain.b, chain.Sigma_x))
    m, P = (v.to(DEV) for v in spring.initial(burn, step, chain))
    H = torch.eye(4, dtype=torch.float64, device=DEV)[:1]
    R = sigma ** 2 * torch.eye(1, dtype=torch.float64, device=DEV)
    eye = torch.eye(4, dtype=torch.float64, device=DEV)
    y = y.double().to(DEV)
    T = (len(y) - 1) * step
    mf, Pf = [], []
    for i in range(T + 1):
        if i:
            m, P = A @ m + b, A @ P @ A.T + Q
        if i % step == 0:
            S = H @ P @ H.T + R
            K = torch.linalg.solve(S, H @ P).T
            m = m + K @ (y[i // step] - H @ m)
            IKH = eye - K @ H
            P = IKH @ P @ IKH.T + K @ R @ K.T
        mf.append(m)
        Pf.append(0.5 * (P + P.T))
    out = torch.empty(samples, T + 1, 4, device=DEV, dtype=torch.float32)
    x = mf[T] + torch.randn(samples, 4, dtype=torch.float64, device=DEV) @ torch.linalg.cholesky(Pf[T]).T
    out[:, T] = x
    for i in range(T - 1, -1, -1):
        Pn = A @ Pf[i] @ A.T + Q
        G = torch.linalg.solve(Pn, A @ Pf[i]).T
        C = Pf[i] - G @ A @ Pf[i]
        L = torch.linalg.cholesky(0.5 * (C + C.T))
        x = mf[i] + (x - (A @ mf[i] + b)) @ G.T + torch.randn(samples, 4, dtype=torch.float64, device=DEV) @ L.T
        out[:, i] = x
    return out


def dense_score(score, x, t):
    """eps by a dense float64 solve on the device."""
    from tests import lgss_ref
    from tests import lgss_util as U
    A, b, Q, m0, P0 = U.spring_case(step=1)[:5]
    L = score.length
    Lam = torch.from_numpy(lgss_ref.precision(A, Q, P0, L - 1)).to(DEV)
    m = torch.from_numpy(lgss_ref.joint(A, b, Q, m0, P0, L - 1)[0]).to(DEV)
    eye = torch.eye(len(m), dtype=torch.float64, device=DEV)

    def run():
        mu, sigma = score._schedule(t).double()
        M = mu ** 2 * eye + sigma ** 2 * Lam
        return (sigma * (Lam @ torch.linalg.solve(M, (x.double().reshape(len(x), -1) - mu * m).T)).T).float().reshape(x.shape)
    return run


def main():
    result = {'device': torch.cuda.get_device_name(0), 'blocks': BLOCKS, 'reps_per_block': REPS}
    chain = spring.make_chain()
    for name, (N, step) in {'posterior_N65_step1': (65, 1), 'posterior_N9_step8': (9, 8)}.items():
        torch.manual_seed(0)
        x = chain.trajectory(chain.prior((1,), device=DEV), 64 + N * step, seed=1)[64 + step - 1::step, 0]
        y = (OBS(x) + 0.05 * torch.randn(N, 1, device=DEV)).float()
        result[name] = alternate({'device': lambda: spring.posterior(y, OBS, 0.05, step, 16384, seed=3),
                                  'torch_ops': lambda: torch_posterior(y, 0.05, step, 16384)})
        exact = spring.posterior(y, OBS, 0.05, step, 16384, seed=3)
        mean = spring.posterior_moments(y, OBS, 0.05, step)[0].to(DEV)
        from sda_amd.metrics import bpf
        from torch.distributions import Normal
        x0 = chain.trajectory(chain.prior((16384,), device=DEV), 64, last=True, seed=5)
        lik = lambda yi, xi: torch.softmax(Normal(yi, 0.05).log_prob(OBS(xi)).sum(dim=-1), 0)  # noqa: E731
        pf = bpf(x0, y, chain.transition, lik, step)[:, step:]
        result[name]['bpf_mean_error'] = float((pf.double().mean(0) - mean).abs().max())
        result[name]['exact_mean_error'] = float((exact.double().mean(0) - mean).abs().max())
        result[name]['bpf_emd_first_512'] = float(metrics.emd(pf[:512].reshape(512, -1), exact[:512].reshape(512, -1)))
    score = spring.ExactScore(chain, 65)
    xs = torch.randn(1024, 65, 4, device=DEV)
    t = torch.tensor(0.5, device=DEV)
    result['exact_score_b1024_L65'] = alternate({'device': lambda: score(xs, t), 'torch_dense_solve': dense_score(score, xs, t)})
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'lgss_bench.json'), 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
