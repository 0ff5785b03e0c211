"""float64 restatement, in plain torch, of what csrc/net1d_train.hip forms -- the weight, bias and modulation gradients of a
single-level 1-D U-Net -- and the case builders its host and device tests share."""
import ctypes

import torch
import torch.nn.functional as F

from sda_amd._lib import NET1D_MAXB, Net1dDesc, Net1dPackDesc, Net1dWgradDesc

ACTS = {0: lambda v: v, 1: F.silu, 2: torch.relu, 3: F.elu, 4: F.gelu, 5: F.selu}
TOL = 1e-4                                   # the training route's own bound: max error <= TOL * max |ref| per tensor


def conv64(x, w, b, circular):
    xp = F.pad(x, (1, 1), mode='circular' if circular else 'constant')
    return F.conv1d(xp, w, b)


def net64(x, ws, bs, mods, circular, act, eps, unbiased):
    """The net in float64 (sda/nn.py:184-206 with one level).  x (n, cin, L); ws / bs in forward order; mods[k] (n or 1, c).
    Returns (out, conv_outs): the output of every convolution in forward order, each retaining its gradient."""
    outs = []

    def conv(v, i):
        y = conv64(v, ws[i], bs[i], circular)
        if y.requires_grad:
            y.retain_grad()
        outs.append(y)
        return y
    a = conv(x, 0)
    for k in range((len(ws) - 2) // 2):
        u = a + mods[k][:, :, None]
        var, mean = torch.var_mean(u, dim=1, unbiased=bool(unbiased), keepdim=True)
        xh = (u - mean) / torch.sqrt(var + eps)
        z = conv(xh, 1 + 2 * k)
        a = a + conv(ACTS[act](z), 2 + 2 * k)
    return conv(a, len(ws) - 1), outs


def conv_grads64(G, U, circular):
    """dw[co][ci][tap] = sum_{n,x} G[n][co][x] U[n][ci][x + tap - 1], db[co] = sum G, in float64."""
    G, U = G.double(), U.double()
    Up = F.pad(U, (1, 1), mode='circular' if circular else 'constant')
    L = G.shape[-1]
    dw = torch.stack([torch.einsum('nox,nix->oi', G, Up[:, :, tap:tap + L]) for tap in range(3)], dim=-1)
    return dw, G.sum((0, 2))


# ------------------------------------------------------------------------------------------------ random saved tensors

def random_saved(cfg, device='cpu', seed=0):
    """What a forward / VJP pair would have left behind, drawn at random (the weight gradient is linear in G and reads U through
    fixed formulas: any values exercise it).  cfg: circular, n, len, cin, c, cout, nb, act, per_image, channel_last, tiles."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    n, L, cin, c, cout, nb = cfg['n'], cfg['len'], cfg['cin'], cfg['c'], cfg['cout'], cfg['nb']
    tiles = cfg.get('tiles', 3)
    t = dict(cfg=cfg)
    t['x'] = r(n, L, cin).permute(0, 2, 1) if cfg.get('channel_last') else r(n, cin, L)
    t['gout'] = r(n, L, cout).permute(0, 2, 1) if cfg.get('channel_last') else r(n, cout, L)
    t['a'], t['z'] = r(max(nb, 1), n, c, L), r(max(nb, 1), n, c, L)
    t['mean'], t['rstd'] = 0.3 * r(max(nb, 1), n, L), torch.rand(max(nb, 1), n, L, generator=g) + 0.5
    t['mod'] = r(n if cfg.get('per_image') else 1, max(nb, 1) * c)
    t['tail_in'] = r(n, c, L)
    t['g_save'] = r(2 * nb + 1, n, c, L)
    t['mod_part'] = r(max(nb, 1), n, tiles, c)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in t.items()}


def reference_grads(t):
    """float64 (dw, db) per convolution in forward order and the modulation gradients (nb, rows, c)."""
    cfg = t['cfg']
    n, L, c, nb, circ = cfg['n'], cfg['len'], cfg['c'], cfg['nb'], cfg['circular']
    cpu = {k: (v.detach().double().cpu() if torch.is_tensor(v) else v) for k, v in t.items()}
    out = [conv_grads64(cpu['g_save'][2 * nb], cpu['x'], circ)]
    for k in range(nb):
        mod = cpu['mod'][:, k * c:(k + 1) * c][:, :, None]
        # the operand as the forward formed it in fp32: (a + mod - mean) rstd -- restated in float64 from the same fp32 inputs
        u = (cpu['a'][k] + mod - cpu['mean'][k][:, None, :]) * cpu['rstd'][k][:, None, :]
        out.append(conv_grads64(cpu['g_save'][2 * k + 1], u, circ))
        out.append(conv_grads64(cpu['g_save'][2 * k], ACTS[cfg['act']](cpu['z'][k]), circ))
    out.append(conv_grads64(cpu['gout'], cpu['tail_in'], circ))
    part = cpu['mod_part'][:nb].sum(2)                    # (nb, n, c)
    dmod = part if cfg.get('per_image') else part.sum(1, keepdim=True)
    return out, dmod


def wgrad_desc(t, slabs=0, frozen=()):
    """-> (descriptor, outputs dict, keep-alive list).  frozen: convolution indices whose dw / db stay NULL."""
    cfg = t['cfg']
    n, L, cin, c, cout, nb = cfg['n'], cfg['len'], cfg['cin'], cfg['c'], cfg['cout'], cfg['nb']
    dev = t['x'].device
    d = Net1dWgradDesc()
    e = d.net
    e.n, e.len, e.cin, e.c, e.cout, e.nblocks = n, L, cin, c, cout, nb
    e.circular, e.act, e.unbiased, e.eps = int(cfg['circular']), cfg['act'], int(cfg.get('unbiased', 1)), 1e-5
    e.x, e.x_sn, e.x_sc, e.x_sx = t['x'].data_ptr(), t['x'].stride(0), t['x'].stride(1), t['x'].stride(2)
    e.a_save, e.z_save, e.save_stride = t['a'].data_ptr(), t['z'].data_ptr(), n * c * L
    e.mean_save, e.rstd_save, e.stat_stride = t['mean'].data_ptr(), t['rstd'].data_ptr(), n * L
    keep = []
    for k in range(nb):
        mk = t['mod'][:, k * c:]
        keep.append(mk)
        e.mod[k] = mk.data_ptr()
    e.mod_sn = t['mod'].stride(0) if cfg.get('per_image') else 0
    d.tail_in = t['tail_in'].data_ptr()
    d.g_save, d.g_stride = t['g_save'].data_ptr(), n * c * L
    go = t['gout']
    d.gout, d.gout_sn, d.gout_sc, d.gout_sx = go.data_ptr(), go.stride(0), go.stride(1), go.stride(2)
    d.mod_part, d.mod_tiles = t['mod_part'].data_ptr(), t['mod_part'].shape[2]
    nconv = 2 + 2 * nb
    shapes = [(c, cin)] + [(c, c)] * (2 * nb) + [(cout, c)]
    # one guard row around every output: nothing outside the unpadded extents may be written
    dws = [torch.full((o + 2, i, 3), 7.0, device=dev) for o, i in shapes]
    dbs = [torch.full((o + 2,), 7.0, device=dev) for o, _ in shapes]
    for v in range(nconv):
        if v not in frozen:
            d.dw[v], d.db[v] = dws[v][1:].data_ptr(), dbs[v][1:].data_ptr()
    rows = n if cfg.get('per_image') else 1
    dmod = torch.full((rows + 2, max(nb, 1) * c + 1), 7.0, device=dev)
    for k in range(nb):
        d.dmod[k] = dmod[1:, k * c:].data_ptr()
    d.dmod_sn = dmod.stride(0)
    d.slabs = slabs
    return d, dict(dw=dws, db=dbs, dmod=dmod), keep


def run_wgrad(t, fn_work, fn_run, slabs=0, frozen=()):
    """fn_work(desc) -> floats of work; fn_run(desc) -> rc.  Returns (dw list, db list, dmod (nb, rows, c)) with the guards checked."""
    d, out, keep = wgrad_desc(t, slabs, frozen)
    floats = int(fn_work(ctypes.byref(d)))
    assert floats > 0, f'planner rc = {floats}'
    work = torch.full((floats,), float('nan'), device=t['x'].device)       # (an unwritten slab would show)
    d.work = work.data_ptr()
    rc = fn_run(d)
    assert rc == 0, f'rc = {rc}'
    cfg = t['cfg']
    nb, c = cfg['nb'], cfg['c']
    dws, dbs = [], []
    for v, (w, b) in enumerate(zip(out['dw'], out['db'])):
        assert (w[0] == 7).all() and (w[-1] == 7).all() and b[0] == 7 and b[-1] == 7, f'convolution {v}: a guard row was written'
        if v in frozen:
            assert (w == 7).all() and (b == 7).all(), f'convolution {v} is frozen and was written'
        dws.append(w[1:-1].clone())
        dbs.append(b[1:-1].clone())
    dm = out['dmod']
    assert (dm[0] == 7).all() and (dm[-1] == 7).all() and (dm[:, nb * c:] == 7).all(), 'modulation gradient: a guard was written'
    dmod = dm[1:-1, :nb * c].reshape(-1, nb, c).permute(1, 0, 2).clone() if nb else dm[1:-1, :0].reshape(0, dm.shape[0] - 2, c)
    return dws, dbs, dmod


def check_against(ref, got, what=''):
    (ref_convs, ref_dmod), (dws, dbs, dmod) = ref, got
    for v, (rw, rb) in enumerate(ref_convs):
        for name, r, g in (('dw', rw, dws[v]), ('db', rb, dbs[v])):
            err = (g.double().cpu() - r).abs().max().item()
            assert err <= TOL * r.abs().max().item() + 1e-12, f'{what} conv {v} {name}: {err:.3e} vs scale {r.abs().max().item():.3e}'
    if ref_dmod.numel():
        err = (dmod.double().cpu() - ref_dmod).abs().max().item()
        assert err <= TOL * ref_dmod.abs().max().item() + 1e-12, f'{what} dmod: {err:.3e}'


# ------------------------------------------------------------------------------------------------ packings

def pack_desc(ws, bs, cin, c, cout, cin_keep, wf, wb, bias):
    p = Net1dPackDesc()
    p.nblocks, p.cin, p.c, p.cout, p.cin_keep = (len(ws) - 2) // 2, cin, c, cout, cin_keep
    for v, (w, b) in enumerate(zip(ws, bs)):
        p.w[v], p.b[v] = w.data_ptr(), None if b is None else b.data_ptr()
    p.wf, p.wb, p.bias = (None if x is None else x.data_ptr() for x in (wf, wb, bias))
    return p
