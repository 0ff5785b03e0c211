"""Reference of one k = 3, stride-1, 1-D launch of sda_conv_igemm (the launches csrc/conv_small1d.hip serves), written from the meaning
of sda_conv_desc in include/sda_hip.h, not from the kernel:

    x[n][ci][p]  = store[(m / n_inner) x_sn_outer + (m % n_inner) x_sn_inner + ci x_sc + p x_sx],  m = n + x_n_off      source view
    v            = x + mod[n mod_sn + ci]                                                                               modulation
    v            = (v - ln_mean[n][p]) ln_rstd[n][p]                                                     LayerNorm, given statistics
    v            = act_in(v)                                                                                     loader activation
    V            = v padded by one position each side, circularly or with zeros                                            padding
    out[n][co][p] = sum_{tap, ci} W[tap][ci][co] V[n][ci][p + tap]                                           3-tap convolution
                    + bias[co]                                                                                                bias
    out         *= act_d'(dact_z)                                                                                        x act'(z)
    out         += res                                                                                                    residual

ln_mean / ln_rstd / mod / dact_z / res / out are indexed by the launch's own image number n: x_n_off moves the source only.

`small1d_ref(launch, dtype)` evaluates these steps in `dtype`: float64 is the reference, float32 (the same steps on the CPU) the
yardstick the GPU tolerance is derived from.  `make_launch(case)` draws the operands of a tests/small1d_cases.py case."""
import torch
import torch.nn.functional as F

from tests import small1d_cases as K

ACTS = {'none': lambda v: v, 'SiLU': F.silu, 'ReLU': F.relu, 'ELU': F.elu, 'GELU': F.gelu, 'SELU': F.selu}
LN_EPS = 1e-5


def pack_logical(w, transpose):
    """W[tap][ci][co] of sda_pack_conv_weight without the padding, from a torch Conv1d weight [cout][cin][3]: forward
    W[tap][ci][co] = w[co][ci][tap]; backward data W[2 - tap][co][ci] = w[co][ci][tap] (the launch's input channels are the layer's
    outputs)."""
    return w.flip(2).permute(2, 0, 1).contiguous() if transpose else w.permute(2, 1, 0).contiguous()


def source_view(store, f):
    """[n][cx][ws] gathered from the flat source storage through the descriptor's source fields `f`."""
    m = torch.arange(f['n'], dtype=torch.int64) + f['x_n_off']
    base = torch.div(m, f['n_inner'], rounding_mode='floor') * f['x_sn_outer'] + (m % f['n_inner']) * f['x_sn_inner']
    idx = (base[:, None, None] + torch.arange(f['cx'], dtype=torch.int64)[None, :, None] * f['x_sc'] +
           torch.arange(f['ws'], dtype=torch.int64)[None, None, :] * f['x_sx'])
    return store.reshape(-1)[idx]


def dact(name, z):
    """act'(z) in z's dtype (autograd of the activation)."""
    if name == 'none':
        return torch.ones_like(z)
    zz = z.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad(ACTS[name](zz).sum(), zz)
    return g


def conv3(v, w, circular):
    """v: [n][cin][ws], w: [3][cin][cout] -> [n][cout][ws]: out[p] = sum_tap w[tap] . V[p + tap], V = v padded by one each side."""
    ws = v.shape[-1]
    vp = torch.cat([v[..., -1:], v, v[..., :1]], dim=-1) if circular else F.pad(v, (1, 1))
    return sum(torch.einsum('io,nip->nop', w[tap], vp[..., tap:tap + ws]) for tap in range(3))


def small1d_ref(L, dtype=torch.float64, lo=0, n=None):
    """The launch `L` (make_launch's dict), images [lo, lo + n), every step in `dtype` -> [n][cout][wo]."""
    n = L['n'] if n is None else n
    c = lambda t: None if t is None else t.to(dtype)
    rows = slice(lo, lo + n)
    v = source_view(c(L['store']), dict(L['src'], n=n, x_n_off=lo))
    if L['mod'] is not None:
        cx = L['src']['cx']
        mod = c(L['mod']).reshape(-1)
        at = (torch.arange(lo, lo + n, dtype=torch.int64) * L['mod_sn'])[:, None] + torch.arange(cx, dtype=torch.int64)[None, :]
        v = v + mod[at][:, :, None]
    if L['ln'] is not None:
        v = (v - c(L['ln'][0])[rows, None, :]) * c(L['ln'][1])[rows, None, :]
    v = ACTS[L['act_in']](v)
    out = conv3(v, c(L['w']), L['circular'])
    if L['bias'] is not None:
        out = out + c(L['bias'])[None, :, None]
    if L['dact_z'] is not None:
        out = out * dact(L['act_d'], c(L['dact_z'])[rows])
    if L['res'] is not None:
        out = out + c(L['res'])[rows]
    return out


def make_launch(case):
    """Seeded float32 CPU operands of a case: dict with `store` (flat source storage), `src` (its descriptor fields), `w_torch` (the
    layer's Conv1d weight), `w` (its logical packing [3][cin][cout]), `b` (the layer's bias or None), and the launch's mod / mod_sn /
    ln / act_in / bias / dact_z / act_d / res (None = off).  The LayerNorm statistics are those of x + mod over the channels
    (unbiased variance, eps 1e-5), computed in float64 and rounded to float32: they are INPUTS of the launch."""
    n, wo, cin, cout = case['n'], case['wo'], case['cin'], case['cout']
    fz = K.FUSIONS[case['fuse']]
    seed = (n * 1009 + wo * 131 + cin * 7 + cout * 3 + int(case['circular']) + 17 * sorted(K.FUSIONS).index(case['fuse']) +
            1000003 * K.VIEWS.index(case['view'])) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    L = dict(case=case, n=n, circular=case['circular'], src=K.source_fields(case))
    L['store'] = rnd(K.source_numel(case))
    if case['transpose']:
        L['w_torch'] = rnd(cin, cout, 3) / (3 * cin) ** 0.5          # Conv1d(cout -> cin): the launch contracts over its outputs
    else:
        L['w_torch'] = rnd(cout, cin, 3) / (3 * cin) ** 0.5
    L['w'] = pack_logical(L['w_torch'], case['transpose'])
    assert tuple(L['w'].shape) == (3, cin, cout)
    assert not (fz['bias'] and case['transpose']), 'a backward-data packing carries no bias'
    L['b'] = rnd(cout) if fz['bias'] else None
    L['bias'] = L['b']
    rows = dict(none=0, shared=1, image=n)[fz['mod']]
    L['mod'] = rnd(rows, cin) if rows else None
    L['mod_sn'] = cin if fz['mod'] == 'image' else 0
    L['ln'] = None
    if fz['ln']:
        x = source_view(L['store'].double(), L['src'])
        if rows:
            x = x + (L['mod'].double()[:, :, None] if rows == n else L['mod'].double()[0][None, :, None])
        var, mean = torch.var_mean(x, dim=1, unbiased=True)
        L['ln'] = (mean.float(), (1.0 / torch.sqrt(var + LN_EPS)).float())
    L['act_in'], L['act_d'] = fz['act'], fz['dact']
    L['dact_z'] = rnd(n, cout, wo) if fz['dact'] != 'none' else None
    L['res'] = rnd(n, cout, wo) if fz['res'] else None
    return L


def yardstick(ref64, ref32):
    """max |float32 evaluation - float64| / max |float64|: the error the same launch makes in float32 on the CPU."""
    return ((ref32.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30)).item()


def tolerance(yard):
    """4 x the float32 CPU evaluation's own error (the margin covers another float32 summation order on the matrix cores), never below
    float32 round-off of the tensor scale (2e-6, assert_close's floor) and never above the project's 1e-4."""
    return min(max(4.0 * yard, 2e-6), 1e-4)
