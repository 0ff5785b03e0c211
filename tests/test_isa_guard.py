"""CPU build-time guard for the hand-scheduled gfx950 kernels (VERDICT r2 item 3 / "what's missing" 5).

conv_wino4's helper waves keep global loads in flight across loop iterations and wait for them with HAND-COUNTED
`s_waitcnt vmcnt(N)` (conv_wino4.hip: W4_WAIT_U / W4_WAIT_HALO): the scheme is only correct while
  * the compiler adds no vector-memory instruction of its own between those waits (a spill reload -- `scratch_load` -- is
    one, and it would also queue behind everything the helpers have in flight), and
  * the number of loads in the program text between two waits is exactly what the counts were derived from.
Nothing on the GPU side fails when that breaks (results stay right if the count errs on the strict side, the kernel just
serialises; on the loose side a register is read before its load landed).  So the device code object hipcc produced for
THIS build is unbundled here (tools/isa_guard.py: clang-offload-bundler + llvm-readelf --notes + llvm-objdump) and checked.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import isa_guard as G  # noqa: E402

LIB = os.path.join(ROOT, 'sda_amd', 'lib')


@pytest.fixture(scope='module')
def built():
    from sda_amd import build as b
    b.build()                                            # incremental: a no-op when the objects are current
    return LIB


def _w4_params(name):
    m = re.search(r'conv_wino4_kernelILb(\d)ELb(\d)ELb(\d)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E', name)
    assert m, name
    mod, ln, silu, epm, var, zp, mf = (int(v) for v in m.groups())
    return bool(mod), bool(ln), bool(silu), epm, var, zp, mf


def test_conv_wino4_no_spills_and_exact_load_counts(built):
    obj = os.path.join(built, 'conv_wino4.o')
    md = G.kernel_metadata(obj)
    dis = G.disassemble(obj)
    kernels = [n for n in md if 'conv_wino4_kernel' in n]
    # the shipped variants: {plain, SiLU, LN} x {no operand, through the helpers, consumer loads} + mod+LN x {none, consumer}
    # + the two zero-position kernels (up-sampled LN + skip launch of the tails, pooled-output launch of their VJP); each for the
    # = 13 for the 96-cout tile (MF = 3).  The 64-cout tile (MF = 2: the reference's default widths, round 6) has no helper-fed operand
    # route (EPM = 1: built, measured slower than the consumers' own loads, removed) and its up-sampled zero-position form takes the skip
    # tensor through consumer-side loads: 10 kernels; the 32-cout tile (MF = 1) has no up-sampled form at all: 9 kernels
    assert len(kernels) == 32, kernels
    seen = set()
    for name in kernels:
        mod, ln, silu, epm, var, zp, mf = _w4_params(name)
        assert var == 0 and mf in (1, 2, 3), f'tooling variant in the product library: {name}'
        seen.add(((mod, ln, silu, epm) if zp == 0 else (mod, ln, silu, epm, zp)) + ((f'mf{mf}',) if mf != 3 else ()))
        k, ins = md[name], dis[name]
        h = G.histogram(ins)
        scratch_ops = sum(v for o, v in h.items() if o.startswith('scratch_'))
        # 8 steps x 4 MF MFMAs x (first | later stage); zero-position kernels: 9 of the 16 positions.  The 64- / 32-cout tiles with an
        # epilogue operand (EPM 2) carry the tile's LAST stage as a third copy: the operand's loads are issued in front of it
        bodies = 3 if (epm == 2 and mf < 3) else 2
        assert sum(v for o, v in h.items() if 'mfma' in o) == bodies * (32 * mf if zp == 0 else 18 * mf), name
        assert k['vgpr_count'] <= 256 and k['agpr_count'] == 0, (name, k)
        if epm in (0, 1):
            # the hot kernels (every launch of the reference nets): nothing spilled, no scratch segment at all
            assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0 and \
                scratch_ops == 0, (name, k, scratch_ops)
        elif mf < 3:
            assert k['vgpr_spill_count'] == 0 and scratch_ops == 0, (name, k, scratch_ops)       # (128 accumulators: room to spare)
        else:
            # the generic consumer-side epilogue (short tiles / two operands; no launch of the reference nets): at most the
            # two entry-time spills the helpers reload once, outside every loop
            assert k['vgpr_spill_count'] <= 2 and scratch_ops <= 4, (name, k, scratch_ops)
        # ---- the hand-counted waits.  Loads per halo set / U slab quarter / prefetch as in the kernel source:
        nsl = 1 if zp == 1 else 3                        # halo slots per lane (up-sampled source: one source pixel per lane)
        nhl = 2 * nsl + (2 * nsl if ln else 0) + (2 if mod else 0)
        # zero-position kernels: the position-packed slab, seven (MF = 3) / five (MF = 2) 1-KiB pieces per helper; full: 4 MF
        nul = {3: 7, 2: 5, 1: 3}[mf] if zp else 4 * mf
        npf = 4 if epm == 1 else 1
        # EPI (MF = 3 only): 6 window slots x 4 + 4 dummies; else: the two arms of one branch
        npf_text = 28 if epm == 1 else 2
        assert epm != 1 or mf == 3, name
        wait_u, wait_halo = nhl + npf, min(63, 2 * (nhl + npf + nul) + nul)
        seq = G.vmem_between_waits(ins)
        if epm == 2:
            continue                                     # (compiler-visible consumer loads interleave their own waits)
        # consumer bias loads, then the helper prologue, then 4 unrolled iterations, then the drain
        assert seq[0] == (0, mf), (name, seq[:3])
        body = seq[4:-1]
        assert len(body) == 8, (name, seq)
        for j in range(4):
            assert body[2 * j] == (wait_u, nhl + npf_text), (name, j, body)       # before W4_WAIT_U: prefetch + halo issue
            assert body[2 * j + 1] == (wait_halo, nul), (name, j, body)           # before W4_WAIT_HALO: the U loads
        assert seq[-1][0] == 0                                                    # final drain
        # no compiler-inserted full drain anywhere else
        assert sum(1 for i in ins if i.startswith('s_waitcnt') and 'vmcnt(0)' in i) == 3, name
    shipped = {(False, False, False, 0), (False, False, False, 1), (False, False, False, 2),
               (False, False, True, 0), (False, False, True, 1), (False, False, True, 2),
               (False, True, False, 0), (False, True, False, 1), (False, True, False, 2),
               (True, True, False, 0), (True, True, False, 2),
               (False, True, False, 1, 1), (False, False, False, 0, 2)}
    assert seen == shipped | {v + ('mf2',) for v in shipped if v[3] != 1} | {(False, True, False, 2, 1, 'mf2')} | \
        {v + ('mf1',) for v in shipped if v[3] != 1}


def test_fused_1d_kernels_have_no_scratch(built):
    for obj, pat in (('block1d.o', 'block1d_'), ('conv_small1d.o', 'conv_small1d_kernel'), ('net1d.o', 'net1d_bwd_kernel'),
                     ('conv_par4.o', 'conv_par4_kernel'), ('conv_few.o', 'conv_few_kernel')):
        md = G.kernel_metadata(os.path.join(built, obj))
        names = [n for n in md if pat in n]
        assert names, obj
        for n in names:
            k = md[n]
            assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
    # the whole-net 1-D kernels, forward and VJP, fused and unfused, all three tile widths: no vector-register spill and not one scratch
    # instruction.  (The forward kernels carry a 20-36 byte private segment -- frame slots of SGPR spills that end up in VGPR lanes
    # (v_writelane / v_readlane), never addressed: the disassembly has no scratch_* / buffer access to it.)
    md = G.kernel_metadata(os.path.join(built, 'net1d.o'))
    dis = G.disassemble(os.path.join(built, 'net1d.o'))
    names = [n for n in md if 'net1d_fwd_kernel' in n or 'net1d_bwd_kernel' in n]
    assert len(names) == 16, names                      # NF = 2 .. 5 (5: whole-sequence tiles of 65 .. 80 positions) x fwd / VJP x fused / unfused
    for n in names:
        assert md[n]['vgpr_spill_count'] == 0, (n, md[n])
        assert not [i for i in dis[n] if 'scratch_' in i], n
        # validity-cone narrowing: blocks 0-2 multiply NF fragments, block 3's LayerNorm too, everything after it NF - 1 (the
        # block body is instantiated three times, the head / tail convolutions in their full and narrow forms)
        assert sum(1 for i in dis[n] if 'v_mfma_f32_16x16x4' in i) > 0
    # the four-class accumulators of conv_par4 (192 registers) must leave room for two waves per SIMD; the multiply loop of a
    # consumer wave issues no vector-memory instruction (a wave that does gets a vmcnt(0) in front of every LDS read)
    md = G.kernel_metadata(os.path.join(built, 'conv_par4.o'))
    par4 = sorted((n, v) for n, v in md.items() if 'conv_par4_kernel' in n)
    assert len(par4) == 3, [n for n, _ in par4]          # cout tile 32 (MT = 1), 64 (MT = 2: the reference's default widths) and 96 (MT = 3)
    for name, k in par4:
        mt = int(re.search(r'conv_par4_kernelILi(\d)E', name).group(1))
        assert k['vgpr_count'] <= 256 and k['agpr_count'] == 0, k
        ins = G.disassemble(os.path.join(built, 'conv_par4.o'))[name]
        assert sum(1 for i in ins if 'mfma' in i) == 36 * mt               # 4 two-channel steps x 9 taps x MT MFMAs, one stage body
        assert sum(1 for i in ins if i.startswith('s_waitcnt') and 'vmcnt(0)' in i) <= 16, 'vmcnt(0) crept into conv_par4'


def test_product_library_has_no_ablation_switches(built):
    """SDA_CONV_DEBUG makes results wrong (it skips loaders / stores for timing experiments): the product build must not
    read it.  The tooling build (-DSDA_ABLATE) does."""
    blob = open(os.path.join(built, 'libsda_hip.so'), 'rb').read()
    assert b'SDA_CONV_DEBUG' not in blob


def test_conv3d_kernel_has_no_spills_and_no_scratch(built):
    """The general 3-D kernel spills nothing and has no scratch access at all."""
    meta = G.kernel_metadata(os.path.join(built, 'conv3d.o'))
    k3 = [v for k, v in meta.items() if 'conv3d_kernel' in k]
    assert len(k3) == 1 and k3[0]['vgpr_spill_count'] == 0 and k3[0]['private_segment_fixed_size'] == 0, k3
    assert not any('scratch_' in t for k, ins in G.disassemble(os.path.join(built, 'conv3d.o')).items() for t in ins)
