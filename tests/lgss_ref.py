"""numpy float64 reference for the linear-Gaussian state space (sda_amd/csrc/lgss.hip), written from the formulas of
include/sda_hip.h with DENSE linear algebra: the joint law of (x_0 .. x_T), Gaussian conditioning on y, the evidence, the exact eps by
numpy.linalg.solve, and a replay of the guided predictor-corrector loop with injected noise."""
import math

import numpy as np


def spring(dt=0.01):
    """A, b, Q, m0, S0 of DampedSpring (sda/mcs.py:60-82), rounded to fp32 as the chain holds them."""
    A = np.array([[1.0, dt, dt ** 2 / 2, 0.0], [0.0, 1.0, dt, 0.0], [-0.5, -0.1, 0.0, 0.2], [0.0, 0.0, 0.0, 0.99]])
    Q = np.diag(np.array([0.1, 0.1, 0.1, 1.0], np.float32) * np.float32(dt))
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return f(A), np.zeros(4), f(Q), np.array([1.0, 0.0, 0.0, 0.0]), np.eye(4)


def random_model(d, k, seed):
    """A random stable chain with a dense observation."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d))
    A *= 0.9 / np.abs(np.linalg.eigvals(A)).max()
    W = rng.standard_normal((d, d))
    Q = W @ W.T / d + 0.1 * np.eye(d)
    W = rng.standard_normal((d, d))
    S0 = W @ W.T / d + 0.5 * np.eye(d)
    return A, rng.standard_normal(d) * 0.1, Q, rng.standard_normal(d), S0, rng.standard_normal((k, d)), rng.standard_normal(k)


def push(A, b, Q, m, P, n):
    for _ in range(n):
        m, P = A @ m + b, A @ P @ A.T + Q
        P = 0.5 * (P + P.T)
    return m, P


def joint(A, b, Q, m0, P0, T):
    """Dense mean ((T + 1) d,) and covariance of (x_0 .. x_T), x_0 ~ N(m0, P0)."""
    d = len(b)
    means, covs = [m0], [P0]
    for _ in range(T):
        means.append(A @ means[-1] + b)
        covs.append(A @ covs[-1] @ A.T + Q)
    C = np.zeros(((T + 1) * d, (T + 1) * d))
    for i in range(T + 1):
        blk = covs[i]
        for j in range(i, T + 1):
            C[i * d:(i + 1) * d, j * d:(j + 1) * d] = blk
            C[j * d:(j + 1) * d, i * d:(i + 1) * d] = blk.T
            blk = blk @ A.T
    return np.concatenate(means), C


def observe(H, c, T, step, d):
    """Dense (N k, (T + 1) d) operator and offset of the observations at indices j step."""
    k = len(c)
    N = T // step + 1
    Hb = np.zeros((N * k, (T + 1) * d))
    for j in range(N):
        Hb[j * k:(j + 1) * k, j * step * d:(j * step + 1) * d] = H
    return Hb, np.tile(c, N)


def condition(mean, cov, Hb, cb, sigma, y):
    """Posterior mean, covariance and log p(y) of y = Hb x + cb + N(0, sigma^2 I), y flat."""
    S = Hb @ cov @ Hb.T + sigma ** 2 * np.eye(len(cb))
    S = 0.5 * (S + S.T)
    r = y - (Hb @ mean + cb)
    K = np.linalg.solve(S, Hb @ cov).T
    pm = mean + K @ r
    pc = cov - K @ Hb @ cov
    _, logdet = np.linalg.slogdet(S)
    logz = -0.5 * (r @ np.linalg.solve(S, r) + logdet + len(cb) * math.log(2 * math.pi))
    return pm, 0.5 * (pc + pc.T), logz


def precision(A, Q, P0, T):
    """Dense block-tridiagonal precision of (x_0 .. x_T)."""
    d = A.shape[0]
    Qi, Si = np.linalg.inv(Q), np.linalg.inv(P0)
    L = np.zeros(((T + 1) * d, (T + 1) * d))
    for i in range(T + 1):
        blk = (Si if i == 0 else Qi) + (A.T @ Qi @ A if i < T else 0)
        L[i * d:(i + 1) * d, i * d:(i + 1) * d] = blk
        if i < T:
            L[i * d:(i + 1) * d, (i + 1) * d:(i + 2) * d] = -A.T @ Qi
            L[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d] = -Qi @ A
    return 0.5 * (L + L.T)


def eps_dense(x, mu, sigma, Lam, m):
    """eps = sigma Lam (mu^2 I + sigma^2 Lam)^-1 (x - mu m) for x (n, (T + 1) d)."""
    M = mu ** 2 * np.eye(len(m)) + sigma ** 2 * Lam
    return sigma * (Lam @ np.linalg.solve(M, (x - mu * m).T)).T


def tables_posterior(table, d, k, T, step, A, b, H, c, m0, y):
    """Compose the sda_lgss_tables slabs into the posterior mean ((T + 1) d,) and the full covariance: the filter means from the
    gains, then the backward kernel x_i | x_{i+1} ~ N(mean_i + G_i (x_{i+1} - A mean_i - b), L_i L_i^T) chained from T down."""
    stride = d * k + 2 * d * d + k * k + 1
    tab = table.reshape(T + 1, stride)
    K = tab[:, :d * k].reshape(T + 1, d, k)
    G = tab[:, d * k:d * k + d * d].reshape(T + 1, d, d)
    L = tab[:, d * k + d * d:d * k + 2 * d * d].reshape(T + 1, d, d)
    Ls = tab[:, d * k + 2 * d * d:d * k + 2 * d * d + k * k].reshape(T + 1, k, k)
    logdet = tab[:, -1]
    mf, logz = [], 0.0
    m = m0
    for i in range(T + 1):
        if i:
            m = A @ m + b
        if i % step == 0:
            v = y[i // step] - (H @ m + c)
            w = np.linalg.solve(Ls[i], v)
            logz += -0.5 * (w @ w + logdet[i] + k * math.log(2 * math.pi))
            m = m + K[i] @ v
        mf.append(m)
    ms = [None] * (T + 1)
    ms[T] = mf[T]
    C = np.zeros(((T + 1) * d, (T + 1) * d))
    C[T * d:, T * d:] = L[T] @ L[T].T
    for i in range(T - 1, -1, -1):
        ms[i] = mf[i] + G[i] @ (ms[i + 1] - (A @ mf[i] + b))
        # x_i = G_i x_{i+1} + independent noise: Cov(x_i, x_j) = G_i Cov(x_{i+1}, x_j) for j > i
        row = G[i] @ C[(i + 1) * d:(i + 2) * d, (i + 1) * d:]
        C[i * d:(i + 1) * d, (i + 1) * d:] = row
        C[(i + 1) * d:, i * d:(i + 1) * d] = row.T
        C[i * d:(i + 1) * d, i * d:(i + 1) * d] = G[i] @ C[(i + 1) * d:(i + 2) * d, (i + 1) * d:(i + 2) * d] @ G[i].T + L[i] @ L[i].T
    return np.concatenate(ms), C, np.stack(mf), logz


def vp(t, eta=1e-3):
    """mu(t), sigma(t) of VPSDE's default 'cos' schedule."""
    a = math.cos(math.acos(math.sqrt(eta)) * t) ** 2
    return a, math.sqrt(1 - a * a + eta * eta)


def pc_replay(x, steps, corrections, tau, noise, score, dtype, eta=1e-3):
    """The predictor-corrector loop of sda/score.py:243-263 in torch on the CPU at `dtype` (float64: the oracle; float32: the yardstick
    of the project's 4x rule), x (n, L, d), the corrector noise taken from noise[step * corrections + j]; score(x, t) is the guided eps."""
    import torch
    x = x.to(dtype)
    dt = 1 / steps
    time = torch.linspace(1, 0, steps + 1, dtype=dtype)
    for i in range(steps):
        t = time[i]
        mu_t, sg_t = vp_torch(t, eta)
        mu_n, sg_n = vp_torch(t - dt, eta)
        r = mu_n / mu_t
        x = r * x + (sg_n - r * sg_t) * score(x, t)
        for j in range(corrections):
            z = noise[i * corrections + j].to(dtype)
            eps = score(x, t - dt)
            delta = tau / eps.square().mean(dim=(1, 2), keepdim=True)
            x = x - (delta * eps + torch.sqrt(2 * delta) * z) * sg_n
    return x


def vp_torch(t, eta=1e-3):
    import torch
    a = torch.cos(math.acos(math.sqrt(eta)) * t) ** 2
    return a, (1 - a ** 2 + eta ** 2).sqrt()


def guided_score(Lam, m, y, std, gamma, sel, dtype, eta=1e-3, dps_zeta=None):
    """GaussianScore (sda/score.py:347-396) -- or DPSGaussianScore (305-344) with dps_zeta -- around the exact eps with the observation
    x[..., sel[0], sel[1]], dense, in torch on the CPU at `dtype`: eps - sigma s, s the gradient through x_hat = (x - sigma eps) / mu."""
    import torch
    n2 = len(m)
    Lam = torch.as_tensor(Lam, dtype=dtype)
    m = torch.as_tensor(m, dtype=dtype)
    y = torch.as_tensor(y, dtype=dtype)

    def score(x, t):
        mu, sigma = vp_torch(t, eta)
        shape = x.shape
        M = mu ** 2 * torch.eye(n2, dtype=dtype) + sigma ** 2 * Lam
        J = sigma * (Lam @ torch.linalg.inv(M))                 # eps = J (x - mu m), J symmetric
        xf = x.reshape(shape[0], n2)
        eps = (xf - mu * m) @ J.T
        xh = ((xf - sigma * eps) / mu).reshape(shape)
        err = y - xh[:, sel[0], sel[1]]
        g = torch.zeros(shape, dtype=dtype)
        if dps_zeta is None:
            g[:, sel[0], sel[1]] = err / (std ** 2 + gamma * (sigma / mu) ** 2)
        else:
            g[:, sel[0], sel[1]] = 2 * err * dps_zeta / err.square().sum().sqrt()
        gf = g.reshape(shape[0], n2)
        s = (gf - sigma * (gf @ J)) / mu                         # (I - sigma J)^T g / mu
        return (eps - sigma * s).reshape(shape)

    return score
