"""Kernel-level numerics of the fp32 detector's neck and head, one launch at a time through rt_debug_fpn against the fp64
references of tests/fpn_kernel_ref.py (plain numpy on the materialised tensors; its docstring derives every bound from the suite's
stage bound U (T + 8) S + 4 U |y|, and tests/test_fpn_kernel_checks_cpu.py proves on the CPU that the checks refuse twenty
plausible errors and that a float32 computation, in the plain form and in the kernels' own, passes them).

Operands are uniform(-1, 1) float32 with full significands, conv weights scaled by 4 / sqrt(K), biases random per channel, scales
in (0.5, 1.5) differing per image and channel.  Every batch is ragged and every launch writes into buffers filled with
RT_DEBUG_CANARY with 64 spare rows; every element of every returned buffer is checked: against the reference inside the op's
output, bit for bit against the canary outside it (the spare rows, the pool tiles an image does not have), +0 in the composed
weights' pad columns.  The rms rule: a kernel's rms error is within twice that of the float32 numpy stand-in of the plain form.

Cases (fpn_kernel_ref.CASES; the instance / route is asserted from the entry's report):
  phase-340 / 540   k_fpn_phase<3, 4, 0> / <5, 4, 0>: an inp conv with given per-image Wf, bias, pool sums; fine images (40, 24), (8, 8),
                    (16, 16), (24, 56) / (4, 4), (12, 20), (36, 20), (16, 32): partial tiles in both axes, an image below a tile, an
                    exact tile, several tiles, a grid sized by another image than the one checked.  540 reads 18 channels in rows
                    of 20 whose pad channels hold noise: a second launch with other noise must return the same bits.
  phase-611 / 610   the head conv with both scale tables and ReLU on the first batch plus (72, 64): <6, 1, 1> with G from a class
                    tensor built in fp64 and rounded; <6, 1, 0> with a bias and no G -- no shipped graph takes this instance; it
                    separates the fine and coarse parts from the gather.
  class-plain / lower   both calls of the net: without lower, bias or scale on (5, 3), (1, 1), (17, 16), (2, 2); with all three on
                    (18, 16), (2, 2), (10, 6), (6, 14) over a lower level of exactly half.  All nine planes, plane stride = batch total.
  compose-12 / 18   three images with different scale rows; pad columns +0.
  chain-compose-phase-12 / 18   compose and phase in one call, against conv3x3(lateral(c) * s + up2(in)).
  inp chain         se_projected -> compose -> phase -> se_tiles for cin 12 and 18 against the plain mathematics, each intermediate
                    table asserted: the composed weights and the output against the fp64 scales (the measured table's bound
                    carried into the weights' bound), the final scales against the fp64 channel means of the reference output.
  head chain        class (p5) -> class (p4) -> phase against the fp64 conv over concat(up8(p5) s5, up4(p4) s4, up2(p3) s3, p2 s2).
  head_fused, conv3 the launch-series forms on the head chain's inputs and the same reference: k_conv3_few<6, 1> gathering the four
                    levels, k_conv3_few<6, 0> (conv_sp, route asserted) on the tensor materialised in float32.
  lateral_add       cin 12 / 18 with b, cin 42 / 12 without; images of 1, 2, 3 and 0 pixels modulo 4.
  upsample_add      with a scale in place on a; without, into a fresh buffer.
  se_projected, se_tiles   images of one pixel, of 192 pixels (two pooling chunks of 128) and in between / the tile grid of the first
                    batch with the canary in the tiles an image does not have.
  tail              1/4-level images (8, 8), (1, 1), (16, 20), (7, 37) = 259 pixels (a partial wave, waves wholly past the smaller
                    images), logits over about +-12; all 16 output pixels per input pixel, the spare blocks intact.
  repeatability     each pooled phase case twice, bit-identical, pool sums included.

The rms rule holds per output buffer: the conv output, the pool sums and the composed weights of a launch each on their own.
What was measured on an MI355X, per case and per buffer, is in docs/HISTORY.md ("the det neck and head kernels against fp64")."""
import numpy as np
import pytest

import fpn_kernel_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_session):
    return hip_session._hd.lib, hip_session._hd.h


def run(dev, c, ins=None):
    """one rt_debug_fpn call for the case (ins: other operand arrays for the same slots); the returned buffers in the order of
    c.reference(), and the entry's report"""
    import ctypes as C
    lib, h = dev
    op, ip, fp, fine, coarse, cins = c.args()
    if ins is not None:
        cins = list(ins) + [None] * (10 - len(ins))
    i = np.zeros(8, np.int32); i[:len(ip)] = ip   # noqa: E702
    f = np.zeros(4, np.float32); f[:len(fp)] = fp   # noqa: E702
    g = [np.array(v, np.int32) for v in ([a for a, _ in fine], [b for _, b in fine], [a for a, _ in coarse], [b for _, b in coarse])]
    arrs = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in cins]
    ptrs = (C.c_void_p * 10)(*[a.ctypes.data if a is not None else None for a in arrs])
    lens = (C.c_longlong * 10)(*[a.size if a is not None else 0 for a in arrs])
    refs = c.reference()
    outs = {o.slot: np.zeros(o.shape, np.float32) for o in refs}
    optrs = (C.c_void_p * 3)(*[outs[k].ctypes.data if k in outs else None for k in range(3)])
    olens = (C.c_longlong * 3)(*[outs[k].size if k in outs else 0 for k in range(3)])
    info = (C.c_int * 1)()
    rc = lib.rt_debug_fpn(h, op, i.ctypes.data, f.ctypes.data, g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, g[3].ctypes.data,
                          len(fine), ptrs, lens, optrs, olens, info)
    assert rc == 0, lib.rt_last_error(h)
    return [outs[o.slot] for o in refs], int(info[0])


def report(case_id, c, fig, info):
    print("FIG %s instance=%s %s" % (case_id, R.INSTANCE_NAMES.get(info, info), " ".join("%s=%.4g" % kv for kv in sorted(fig.items()))))


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_fpn_kernel_against_fp64(dev, case_id):
    c = R.case(case_id)
    outs, info = run(dev, c)
    assert info == c.info, "%s ran on %s" % (c.name, R.INSTANCE_NAMES.get(info, info))
    report(case_id, c, R.check(c, outs), info)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_phase_output_does_not_depend_on_the_pad_channels(dev):
    c = R.case("phase-540")
    first, _ = run(dev, c)
    ins = c.ins
    ins[0] = c.with_noise(99)
    assert not np.array_equal(ins[0], c.x) and np.array_equal(ins[0][:, :18], c.x[:, :18])
    second, _ = run(dev, c, ins)
    assert same_bits(first, second)


@pytest.mark.parametrize("case_id", ["phase-340", "phase-540", "chain-compose-phase-12", "chain-compose-phase-18"])
def test_pooled_phase_cases_repeat_bit_for_bit(dev, case_id):
    c = R.case(case_id)
    assert same_bits(run(dev, c)[0], run(dev, c)[0])


@pytest.mark.parametrize("cin,batch", [(12, R.BATCH_A), (18, R.BATCH_B)])
def test_inp_chain_against_the_plain_mathematics(dev, cin, batch):
    """se_projected -> compose -> phase -> se_tiles as DetNet::run issues them for inp0 (cin 12) and inp1 (cin 18), every table a kernel
    leaves fed to the next launch as it is, every reference the fp64 plain form of the whole chain up to that point"""
    n = len(batch)
    ph = R.Phase("inp chain cin %d: compose -> phase" % cin, cin, batch, R.F_BIAS | R.F_POOL | R.F_COMPOSE, 40 + cin)
    sp = R.SeProjected("inp chain cin %d: se_projected" % cin, cin, batch, 50 + cin, x=ph.x, lat=ph.lat)
    (table,), _ = run(dev, sp)
    report("inp-chain-%d-se_projected" % cin, sp, R.check(sp, [table]), 0)
    s_ref = sp.reference()[0]
    ph.lat_scale = table[:n].copy()
    ph.lat_scale_ref, ph.lat_scale_err = s_ref.v[:n], s_ref.bound[:n]
    outs, info = run(dev, ph)
    assert info == ph.info
    report("inp-chain-%d-phase" % cin, ph, R.check(ph, outs), info)
    y_ref, pool_ref, _ = ph.reference()
    T = R.tiles_alloc(batch)
    st = R.SeTiles("inp chain cin %d: se_tiles" % cin, batch, 60 + cin, pool=outs[1][:n * T])
    off = R.offsets(batch)
    st.ref_mean = np.stack([y_ref.v[off[i]:off[i + 1]].mean(0) for i in range(n)])
    st.ref_dmean = np.stack([np.where(pool_ref.mask[i * T:(i + 1) * T], pool_ref.bound[i * T:(i + 1) * T], 0).sum(0) / (h * w)
                             for i, (h, w) in enumerate(batch)])
    (scale,), _ = run(dev, st)
    report("inp-chain-%d-se_tiles" % cin, st, R.check(st, [scale]), 0)


def test_head_chain_against_the_plain_mathematics(dev):
    """class (p5) -> class (p4) -> phase: one running fp32 sum over three launches, against the fp64 conv over the concatenation"""
    hc = R.case("head_fused")
    l5, l4 = hc.levels[0], hc.levels[1]
    c5 = R.ClassOp("head chain: class p5", l5, 2, 70, w=hc.w, z=hc.p[0], scale=hc.sc[0])
    (v5,), _ = run(dev, c5)
    report("head-chain-class-p5", c5, R.check(c5, [v5]), 0)
    c4 = R.ClassOp("head chain: class p4", l4, 7, 71, w=hc.w, bias=hc.bias, z=hc.p[1], scale=hc.sc[1], lower=v5[:9 * R.pixels(l5)].copy())
    (v45,), _ = run(dev, c4)
    report("head-chain-class-p4", c4, R.check(c4, [v45]), 0)
    ph = R.Phase("head chain: phase", 24, hc.fine, R.F_G | R.F_RELU | R.F_FS | R.F_CS, 72, x=hc.p[3], z=hc.p[2], w=hc.w, fs=hc.sc[3],
                 cs=hc.sc[2], G=v45[:9 * R.pixels(l4)].copy())
    (y,), info = run(dev, ph)
    assert info == 611
    report("head-chain-phase", ph, R.check(ph, [y]), info)          # the launch against its own operands
    report("head-chain", hc, R.check(hc, [y]), info)                # the chain against the plain mathematics
