"""The plan of the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip) by hand, in plain Python, for its three
geometries: the stride-1 block convolutions ('s1'), the up-sampling tails ('tail_up') and the stride-2 heads ('head_s2').  The case
modules tests/wgrad3_cases.py and tests/wgrad3x_cases.py hold it against their tables and against the library's planner."""
S1, UP2, S2 = 's1', 'tail_up', 'head_s2'
LDS_MAX = 160 * 1024


def out_size(kind, h, w):
    return (h // 2, w // 2) if kind == S2 else (h, w) if kind == S1 else (2 * h, 2 * w)       # ('tail_up_plain' is up2 as well)


def pitch(need):
    """The smallest LDS channel pitch >= need that is 2 (mod 32) floats."""
    return (need + 29) // 32 * 32 + 2


def plan(kind, cin, cout, n, h, w, slabs=0):
    """(h, w: the SOURCE size) -> dict(R, nrb, S, mt, n_ct, n_cit, q4, q4_rounds, lds_bytes, per, slabs, vp, gp)."""
    ho, wo = out_size(kind, h, w)
    w2 = wo + 2
    R = min(max(128 // w2, 1), ho)
    nrb = -(-ho // R)
    S = n * nrb
    mt = 3 if cout % 96 == 0 else 2 if cout % 64 == 0 else 1
    n_ct, n_cit = cout // (32 * mt), cin // 32
    q4 = (R * w2 + 3) // 4 * 4
    if kind == S2:                        # four parity planes of R + 1 rows; the last tap reads plane 3 at q4 - 1 + w2 + 1
        vp = pitch(3 * (R + 1) * w2 + q4 + w2 + 1)
    else:                                 # R + 2 rows of the source (s1) or up-sampled (up2) image
        vp = pitch(q4 + 2 * w2 + 2)
    lds = 4 * (32 * vp + 32 * mt * pitch(q4))
    s = slabs or min(512 // (n_ct * n_cit), 256)
    s = max(min(s, S), 1)
    per = -(-S // s)
    return dict(R=R, nrb=nrb, S=S, mt=mt, n_ct=n_ct, n_cit=n_cit, q4=q4, q4_rounds=q4 != R * w2, lds_bytes=lds, per=per,
                slabs=-(-S // per), vp=vp, gp=pitch(q4))
