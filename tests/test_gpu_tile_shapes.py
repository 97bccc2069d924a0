"""-m gpu: every gather-GEMM tile forced (DC_CONV_VARIANT / DC_CONV_VARIANT_BF16) on small nets built so that the paths the 72x104
ResNet-152 of test_gpu_variants.py enters once or not at all are walked: the XCD map of single-problem launches in a two-dimensional
arrangement and with rectangles of two widths (both magic divisions) — reached by EVERY tile size only through the two wide nets,
see XCD_NETS, and asserted per tile from the tile's BM x BN —, parity classes of several m tiles with a ragged n tile in the
multi-class tile map, the same deconvolution as one launch per class (DC_DECONV_MERGE=0), a cropped window + residual + sigmoid
prefix on the merged heads, and classes so small that some XCD rows are empty.  Weights go in through net.params; the reference is
oracle.OracleNet on the CPU.

What a forced tile gets (asserted on plan_text(), so that no tile drops out silently):
  * a tile WITH a multi-class instantiation runs a deconvolution as one launch ("[4 classes]") and, under DC_DECONV_MERGE=0, as four;
  * a tile WITHOUT one keeps the forced tile on four per-class launches in both runs ("a tile without a multi-class
    instantiation gets one launch per class"; net_lower.cpp looks for a multi-class tile among the FORCED candidates before it
    merges, so the cost model's tile never replaces the forced one on a deconvolution);
  * the only layers a forced tile may miss are those of EXCUSED below, which then run on another tile and are still compared.

Compared are the blobs of oracle.OracleNet, with one departure: on the 16-bit heads at fuse=0 the Crop / Eltwise / Sigmoid blobs are
held to the element-wise operation applied to the DEVICE's own bottom blobs (see _check_heads); the (de)convolution blobs, which are
what a tile computes, are compared with the oracle directly in every element type.

Both 16-bit kinds run on operands that ARE values of their format (bf16_round; f16_operands of test_gpu_fp16.py) against the oracle
accumulating in double, and every tile is held to ONE rounding of its output: |got - ref| <= ulp(ref) + 1e-6 x range (_layer_bound) —
for float16 that is every h... and d... tile with split-K 2 and 4, the four epilogues, merged and per-class deconvolutions, the
shortcut through LDS-DMA and the sigmoid prefix.  (Float16 operands that are not float16 values keep the former 2e-3 x range:
test_fp16_single_layers.)  Largest |got - ref| / bound over all tiles and nets, measured on an MI355X: float16 0.499, bfloat16 0.549 —
no float16 row needed more than the 1e-6 x range accumulation term.  Float32 used 0.015 of its 1e-4 x range, which is why its
(de)convolution blobs with their fused epilogue (the four XCD nets, `deconv`, `deconv_tiny`) are ALSO held to the error of a plain float32
sum, tests/f32_ref.py: at most 3 x the maximum and 2 x the RMS error of a sequential float32 sum over K; measured, worst over all
float32 tiles and those nets: 1.13 x the maximum, 1.00 x the RMS.  The `heads` net (sigmoid prefix, cropped residual) keeps the 1e-4 x range alone."""
import os
import re

import numpy as np
import pytest

import f32_ref as F
from oracle import oracle as O
from test_gpu_bf16 import bf16_round, bf16_ulp
from test_gpu_fp16 import f16_operands, f16_ulp
from test_gpu_layers import _inp

pytestmark = pytest.mark.gpu
MAX_TILES, MAX_TILES_BF16 = 64, 40  # parametrisation bounds; indices past a table's end are skipped, a longer table fails

# The tiles that have a multi-class instantiation (11 + 8 + 4 of the 55; the bfloat16 table has the copies of the 8 + 4).
# A literal: a tile that lost its instantiation would otherwise just move to the per-class column without anybody noticing.
MULTI_CLASS = {
    "64x64x32_w221_p3", "64x64x64_w221_p3", "32x64x64_w122_p4", "32x32x128_w114_p3", "32x32x64_w114_p4", "32x64x64_w124_p4",
    "64x64x64_w222_p3", "128x64x32_w222_p2", "128x128x32_w222_p2", "32x32x128_w118_p3", "64x128x32_w222_p2",
    "h128x128x64_w221_p2", "h128x64x64_w221_p2", "h64x64x64_w221_p3", "h64x64x128_w222_p2", "h32x64x128_w122_p3", "h32x64x256_w124_p2",
    "h128x128x128_w222_p2", "h32x32x256_w114_p2",
    "d128x128x64_w221_s2", "d128x128x64_w222_s3", "d256x128x64_w421_s3", "d128x256x64_w241_s3",
}
MULTI_CLASS_BF16 = {
    "b128x128x64_w221_p2", "b128x64x64_w221_p2", "b64x64x64_w221_p3", "b64x64x128_w222_p2", "b32x64x128_w122_p3", "b32x64x256_w124_p2",
    "b128x128x128_w222_p2", "b32x32x256_w114_p2",
    "bd128x128x64_w221_s2", "bd128x128x64_w222_s3", "bd256x128x64_w421_s3", "bd128x256x64_w241_s3",
}

# Tiles that cannot take one of the layers here BY CONSTRUCTION, and the layers that reason covers: name -> (reason, layers).
# "dilated" is the 3x3 layer of net 2, "skip" the 1x1 convolutions on `hi` of net 4: both gather taps of 128 channels.
_BK256 = "BK = 256: one K tile is longer than a tap of 128 input channels (tile_takes_k, net.h)"
EXCUSED = {
    "h32x64x256_w124_p2": (_BK256, {"dilated", "skip"}),
    "h32x32x256_w114_p2": (_BK256, {"dilated", "skip"}),
    "b32x64x256_w124_p2": (_BK256, {"dilated", "skip"}),
    "b32x32x256_w114_p2": (_BK256, {"dilated", "skip"}),
}

HEADS = (14, 28, 44)
WORST = {}  # element type -> largest error / bound seen so far in this process (printed by every test)


@pytest.fixture(autouse=True)
def _tiles_only(monkeypatch):
    for k in ("DC_WINOGRAD", "DC_STREAM1X1", "DC_STEM"):  # the layers stay on the tile: no Winograd, streaming or stem form
        monkeypatch.setenv(k, "0")
    monkeypatch.delenv("DC_DECONV_MERGE", raising=False)


# ---- the nets ---------------------------------------------------------------------------------------------------------------------
def _conv(name, bot, top, cout, k, pad=0, dil=1, stride=1, bias=False, typ="Convolution"):
    return ('layer { name: "%s" type: "%s" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d pad: %d '
            "stride: %d dilation: %d bias_term: %s } }\n" % (name, typ, bot, top, cout, k, pad, stride, dil, "true" if bias else "false"))


def _bn_scale(bot):
    return ('layer { name: "bn" type: "BatchNorm" bottom: "%s" top: "%s" batch_norm_param { use_global_stats: true } }\n'
            'layer { name: "sc" type: "Scale" bottom: "%s" top: "%s" scale_param { bias_term: true } }\n' % (bot, bot, bot, bot))


def _net_text(which):
    if which == "xcd":  # 1: M = 1517 -> 12 x 2 tiles at 128x128, 48 x 8 at 32x32; 256-row and 256-column tiles stay below 16 tiles
        return (_inp("x", (1, 256, 37, 41)) + _conv("c", "x", "c", 256, 1) + _bn_scale("c") +
                'layer { name: "sum" type: "Eltwise" bottom: "x" bottom: "c" top: "y" }\nlayer { name: "re" type: "ReLU" bottom: "y" top: "y" }\n')
    if which == "dilated":  # 2: the same M with a gathered K (9 taps of 128 channels)
        return (_inp("x", (1, 128, 37, 41)) + _conv("c", "x", "y", 128, 3, pad=2, dil=2) + _bn_scale("y") +
                'layer { name: "re" type: "ReLU" bottom: "y" top: "y" }\n')
    if which == "xcd_wide":  # 1 with 672 output channels: 6 x 6 tiles at 256x128, 12 x 3 at 128x256; tiles_n = 21 / 11 / 6 / 3
        return (_inp("x", (1, 256, 37, 41)) + _inp("r", (1, 672, 37, 41)) + _conv("c", "x", "c", 672, 1) + _bn_scale("c") +
                'layer { name: "sum" type: "Eltwise" bottom: "r" bottom: "c" top: "y" }\nlayer { name: "re" type: "ReLU" bottom: "y" top: "y" }\n')
    if which == "dilated_wide":  # 2 with 288 output channels: tiles_n = 9 / 5 / 3 / 2
        return (_inp("x", (1, 128, 37, 41)) + _conv("c", "x", "y", 288, 3, pad=2, dil=2) + _bn_scale("y") +
                'layer { name: "re" type: "ReLU" bottom: "y" top: "y" }\n')
    if which == "deconv":  # 3: classes of 782 .. 864 pixels, Cout = 44 leaves a ragged n tile at every BN
        return _inp("x", (2, 256, 17, 23)) + _conv("up", "x", "y", 44, 3, stride=2, bias=True, typ="Deconvolution")
    if which == "deconv_tiny":  # 3 at batch 1 on 3x2 cells: classes of 6 .. 12 pixels, XCD rows without an m tile in every arrangement
        return _inp("x", (1, 256, 3, 2)) + _conv("up", "x", "y", 44, 3, stride=2, bias=True, typ="Deconvolution")
    assert which == "heads"  # 4: three sibling heads; at fuse=2 ONE 86-channel deconvolution with cropped window, residual, sigmoid prefix
    t = _inp("low", (2, 256, 17, 23)) + _inp("hi", (2, 128, 34, 46))
    for k, n in enumerate(HEADS):
        t += _conv("up%d" % k, "low", "up%d" % k, n, 3, stride=2, bias=True, typ="Deconvolution")
        t += _conv("skip%d" % k, "hi", "skip%d" % k, n, 1, bias=True)
        t += 'layer { name: "crop%d" type: "Crop" bottom: "up%d" bottom: "skip%d" top: "up%dc" }\n' % (k, k, k, k)
        t += 'layer { name: "sum%d" type: "Eltwise" bottom: "skip%d" bottom: "up%dc" top: "sum%d" }\n' % (k, k, k, k)
        if k == 0:
            t += 'layer { name: "prob" type: "Sigmoid" bottom: "sum0" top: "prob" }\n'
    return t


_SEEDS = {"xcd": 11, "dilated": 12, "deconv": 13, "deconv_tiny": 14, "heads": 15, "xcd_wide": 16, "dilated_wide": 17}

# The single-problem nets: name -> (kind for EXCUSED, plan label, M, Cout, Ktot, tap rows, K per tap).  "xcd" and "dilated" are the
# two the tile tests were asked to run; on their own they leave the XCD map OFF for the 256-row / 256-column tiles (12 tiles or
# fewer) and, with 256 and 128 output channels, give every XCD the same rectangle width (tiles_n is a power of two), so only one of
# the two magic divisions of slot / rw is ever used.  The two wide nets are there for that: 672 and 288 output channels.
XCD_NETS = {
    "xcd": ("xcd", "c+bn+sc+sum+re", 1517, 256, 256, 1, 256),
    "dilated": ("dilated", "c+bn+sc+re", 1517, 128, 1152, 3, 128),
    "xcd_wide": ("xcd", "c+bn+sc+sum+re", 1517, 672, 256, 1, 256),
    "dilated_wide": ("dilated", "c+bn+sc+re", 1517, 288, 1152, 3, 128),
}
# Tiles that reach no two-dimensional arrangement, or no arrangement with two rectangle widths, on any of XCD_NETS: name -> reason.
XCD_EXCUSED = {}


def _xcd_arrangement(M, N, Ktot, nty, klen, BM, BN):
    """The XCD arrangement launch_conv_gemm (conv_gemm.cpp) gives a single-problem launch, restated: None when the map stays off (fewer
    than 16 tiles), else (gx, gy, tiles_m, tiles_n, rectangle widths).  plan_text() does not show the arrangement, so this model of the
    host's choice is what the premise of the XCD nets is asserted on; it has to follow the host code if that changes."""
    tm, tn = -(-M // BM), -(-N // BN)
    grid, best, out = tm * tn, 1e300, None
    if grid < 16:
        return None
    for lgx in range(4):
        gx, gy = 1 << lgx, 8 >> lgx
        if gx > tn or gy > tm:
            continue
        rw = [((tn * (q + 1)) >> lgx) - ((tn * q) >> lgx) for q in range(gx)]
        rh = [((tm * (q + 1)) >> (3 - lgx)) - ((tm * q) >> (3 - lgx)) for q in range(gy)]
        cost = (float(N) * Ktot / gx + float(M) * klen * nty / gy) * (1.0 + 0.02 * (max(rw) * max(rh) * 8 - grid) / float(grid))
        if cost < best:
            best, out = cost, (gx, gy, tm, tn, sorted(set(rw)))
    return out


def _check_xcd_premise(tile, excused):
    """What the XCD nets are for, per tile, from its BM x BN: on the nets the tile really runs, at least one launch has the map on
    (>= 16 tiles) in a two-dimensional arrangement with tiles_m >= 2 and tiles_n >= 2, and at least one has rectangles of two widths
    (floor(tiles_n / gx) and floor + 1: both magic divisions).  -> {net: arrangement} for the report."""
    bm, bn = [int(v) for v in re.search(r"(\d+)x(\d+)x\d+", tile).groups()]
    arr = {n: _xcd_arrangement(M, N, K, nty, klen, bm, bn) for n, (kind, _l, M, N, K, nty, klen) in XCD_NETS.items() if kind not in excused}
    on = [a for a in arr.values() if a]
    if tile not in XCD_EXCUSED:
        assert any(gx >= 2 and gy >= 2 and tm >= 2 and tn >= 2 for gx, gy, tm, tn, _ in on), "%s: no two-dimensional XCD arrangement: %s" % (tile, arr)
        assert any(len(rw) == 2 for _gx, _gy, _tm, _tn, rw in on), "%s: no arrangement with two rectangle widths: %s" % (tile, arr)
    return arr


class _Case(object):
    """Inputs, weights and the oracle's blobs of one net in one element kind.  bfloat16 and float16: inputs and (de)convolution filters
    are values of the format (float16: none of them subnormal) and the oracle accumulates in double, as test_bf16_conv_deconv_configs
    and test_fp16_conv_deconv_configs do."""

    def __init__(self, caffe, which, dtype):
        self.which, self.text = which, _net_text(which)
        rs = np.random.RandomState(_SEEDS[which] + {"f32": 0, "bf16": 100, "f16": 200}[dtype])
        q = {"f32": lambda a: np.asarray(a, np.float32), "bf16": bf16_round, "f16": f16_operands}[dtype]
        probe = caffe.Net(self.text, caffe.TEST, from_text=True, fuse=0)  # parameter shapes only; never run
        self.inputs = {n: q(rs.randn(*probe.blobs[n].shape)) for n in probe.inputs}
        self.weights = []
        for name in probe.params:
            shapes = [p.shape for p in probe.params[name]]
            if name == "bn":
                vals = [rs.randn(*shapes[0]) * 0.1, 1 + rs.rand(*shapes[1]), np.ones(1)]
            elif name == "sc":
                vals = [1 + 0.1 * rs.randn(*shapes[0]), 0.1 * rs.randn(*shapes[1])]
            else:  # (de)convolution: unit-variance outputs; the deconvolution's fan-in is Cin x the (at most 4) taps of a class
                fan = shapes[0][1] * shapes[0][2] * shapes[0][3] if not name.startswith("up") else shapes[0][0] * 4
                vals = [q(rs.randn(*shapes[0]) / np.sqrt(fan))] + [rs.randn(*s) for s in shapes[1:]]
            self.weights.append((name, "", [np.asarray(v, np.float32) for v in vals]))
        O.set_threads(min(16, os.cpu_count() or 1))
        O.set_double_acc(dtype != "f32")
        try:
            self.ref = {k: v.copy() for k, v in O.OracleNet(self.text, self.weights).forward(**self.inputs).items()}
        finally:
            O.set_double_acc(False)

    def f32_case(self):
        """(ref64, model32, pixels) of tests/f32_ref.py for the net's (de)convolution with its fused epilogue (float32 cases, not `heads`)"""
        W = {name: blobs for name, _t, blobs in self.weights}
        x = self.inputs["x"]
        if self.which.startswith("deconv"):
            w, bias = W["up"]
            return F.layer_case("deconv", x, w, *F.fold_affine64(w.shape[1], bias), stride=2)
        w = W["c"][0]
        a, b = F.fold_affine64(w.shape[0], None, W["bn"], W["sc"])
        if self.which.startswith("dilated"):
            return F.layer_case("conv", x, w, a, b, None, True, 1, 2, 2)
        return F.layer_case("conv", x, w, a, b, self.inputs["r" if self.which == "xcd_wide" else "x"], True)


@pytest.fixture(scope="module")
def cases(gpu_caffe):
    memo = {}

    def get(which, dtype):
        key = (which, dtype)
        if key not in memo:
            memo[key] = _Case(gpu_caffe, which, dtype)
        return memo[key]

    return get


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def _layer_bound(ref, dtype):
    """What ONE layer may differ by from the oracle's value of it, per element (an array or a scalar).
    f32: 1e-4 of the range (test_gpu_layers.py, test_random_graph); bf16 / f16: one ulp of the format at the reference + 1e-6 of the
    range (test_bf16_conv_deconv_configs, test_fp16_conv_deconv_configs)."""
    rng = float(np.abs(ref).max())
    if dtype == "bf16":
        return bf16_ulp(ref) + 1e-6 * rng
    if dtype == "f16":
        return f16_ulp(ref) + 1e-6 * rng
    return 1e-4 * max(1.0, rng)


def _tight(got, case, dtype, what):
    """float32 runs only: the blob against the float64 reference at the margins of tests/f32_ref.py, beside _hold"""
    if dtype == "f32":
        ref64, model, pixels = case.f32_case()
        F.assert_f32_tight(got, ref64, model, "gather-GEMM tiles (forced): " + what, pixels)


def _hold(got, ref, bound, dtype, what):
    assert got.shape == ref.shape, what
    ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max())
    WORST[dtype] = max(WORST.get(dtype, 0.0), ratio)
    err = float(np.abs(got - ref).max())
    assert ratio <= 1.0, "%s: max |got - ref| = %g, %.3f of the bound" % (what, err, ratio)
    return err / max(1.0, float(np.abs(ref).max()))


# ---- one run ----------------------------------------------------------------------------------------------------------------------
def _run(caffe, case, dtype, fuse, monkeypatch, merge):
    if merge:
        monkeypatch.delenv("DC_DECONV_MERGE", raising=False)
    else:
        monkeypatch.setenv("DC_DECONV_MERGE", "0")
    net = caffe.Net(case.text, caffe.TEST, from_text=True, fuse=fuse, dtype=dtype)
    for name, _t, blobs in case.weights:
        for p, v in zip(net.params[name], blobs):
            p.data[...] = v
    for k, v in case.inputs.items():
        net.blobs[k].data[...] = v
    out = {k: v.copy() for k, v in net.forward().items()}
    if fuse == 0:
        out = {k: net.blobs[k].data.copy() for k in case.ref if k not in case.inputs}
    return out, _plan_of(net)


def _plan_of(net):
    """(tile, label) of every gather-GEMM launch of the net's plan."""
    plan = []
    for ln in net.plan_text().splitlines():
        f = ln.split("\t")
        if len(f) >= 4 and f[1].startswith("conv_gemm<"):
            plan.append((f[1][len("conv_gemm<"):-1], f[3]))
    return plan


def _check_plan(plan, tile, merged_expected, layers, excused):
    """layers: [(label prefix, kind, is a deconvolution)].  Every launch of a layer names the forced tile (another one exactly where
    EXCUSED says so); a deconvolution is ONE launch labelled "[4 classes]" where merged_expected, else four "[class r,c]" launches."""
    for prefix, kind, deconv in layers:
        mine = [(t, lab) for t, lab in plan if lab == prefix or lab.startswith(prefix + " [")]
        if kind in excused:
            assert mine and all(t != tile for t, _ in mine), (tile, kind, mine)
        else:
            assert mine and all(t == tile for t, _ in mine), "%s was not forced on %s: %s" % (tile, prefix, mine)
        if deconv and merged_expected:
            assert len(mine) == 1 and mine[0][1] == prefix + " [4 classes]", mine
        elif deconv:
            assert sorted(lab for _, lab in mine) == ["%s [class %d,%d]" % (prefix, r, c) for r in (0, 1) for c in (0, 1)], mine
        else:
            assert len(mine) == 1, mine
    assert len(plan) == sum(1 if not d else (1 if merged_expected else 4) for _, _, d in layers), plan


_HEAD_FUSED = "+".join("up%d+crop%d+sum%d" % (k, k, k) + ("+prob" if k == 0 else "") for k in range(3))


def _heads_layers(fuse):
    if fuse == 2:
        return [("skip0+skip1+skip2", "skip", False), (_HEAD_FUSED, "deconv", True)]
    return [(n % k, kind, d) for k in range(3) for n, kind, d in (("up%d", "deconv", True), ("skip%d", "skip", False))]


def _check_heads(out, case, dtype, fuse, what):
    """f32: every blob against the oracle's chain.  16 bit: every layer rounds its output, so at fuse=0 each blob is held to the
    per-layer bound against the oracle's layer applied to the DEVICE's own bottom blobs (exactly what the next launch read); the
    (de)convolutions read the net inputs, so theirs are the oracle's.  At fuse=2 the outputs are one launch over `low` plus the skip
    launch's rounded output.  Both 16-bit kinds, whose bound is one ulp of the reference ELEMENT:
    sum_k = rnd(deconv + skip_k'), |skip_k' - skip_k| <= bound(skip_k), and where the two cancel an ulp of skip_k exceeds one of sum_k,
    hence bound(sum_k) + bound(skip_k); the sigmoid's slope is at most 1/4 and sum0 is not rounded in between: bound(prob) +
    bound(skip0) / 4."""
    R, worst = case.ref, 0.0
    if dtype == "f32":
        for k in sorted(out):
            worst = max(worst, _hold(out[k], R[k], _layer_bound(R[k], dtype), dtype, "%s, blob %s" % (what, k)))
        return worst
    if fuse == 0:
        for k in range(3):
            for n in ("up%d" % k, "skip%d" % k):
                worst = max(worst, _hold(out[n], R[n], _layer_bound(R[n], dtype), dtype, "%s, blob %s" % (what, n)))
            crop = O.crop_forward(out["up%d" % k], out["skip%d" % k])
            assert np.array_equal(out["up%dc" % k], crop), "%s, blob up%dc" % (what, k)
            ref = out["skip%d" % k].astype(np.float64) + crop
            worst = max(worst, _hold(out["sum%d" % k], ref, _layer_bound(ref, dtype), dtype, "%s, blob sum%d" % (what, k)))
        ref = 1.0 / (1.0 + np.exp(-out["sum0"].astype(np.float64)))
        return max(worst, _hold(out["prob"], ref, _layer_bound(ref, dtype), dtype, what + ", blob prob"))
    for k, n in ((1, "sum1"), (2, "sum2")):
        bound = _layer_bound(R[n], dtype) + _layer_bound(R["skip%d" % k], dtype)
        worst = max(worst, _hold(out[n], R[n], bound, dtype, "%s, blob %s" % (what, n)))
    bound = _layer_bound(R["prob"], dtype) + 0.25 * _layer_bound(R["skip0"], dtype)
    return max(worst, _hold(out["prob"], R["prob"], bound, dtype, what + ", blob prob"))


def _exercise(caffe, cases, tile, dtype, monkeypatch):
    excused = EXCUSED.get(tile, ("", set()))[1]
    has_mc = tile in MULTI_CLASS or tile in MULTI_CLASS_BF16
    report = {"merged": [], "per class": []}
    errs = []
    # 1, 2 and their wide forms: the XCD map of single-problem launches, dense and gathered K
    arr = _check_xcd_premise(tile, excused)
    for which, (kind, label) in sorted((n, v[:2]) for n, v in XCD_NETS.items()):
        case = cases(which, dtype)
        out, plan = _run(caffe, case, dtype, 2, monkeypatch, True)
        _check_plan(plan, tile, False, [(label, kind, False)], excused)
        errs.append(_hold(out["y"], case.ref["y"], _layer_bound(case.ref["y"], dtype), dtype, "%s, net %s" % (tile, which)))
        _tight(out["y"], case, dtype, "%s, net %s" % (tile, which))
    # 3: the stand-alone deconvolution, full size and tiny, merged and per class
    for which in ("deconv", "deconv_tiny"):
        case = cases(which, dtype)
        outs = {}
        for merge in (True, False):
            out, plan = _run(caffe, case, dtype, 2, monkeypatch, merge)
            _check_plan(plan, tile, merge and has_mc, [("up", "deconv", True)], excused)
            what = "%s, net %s %s" % (tile, which, "merged" if merge else "per class")
            errs.append(_hold(out["y"], case.ref["y"], _layer_bound(case.ref["y"], dtype), dtype, what))
            _tight(out["y"], case, dtype, what)
            report["merged" if merge and has_mc else "per class"].append(which)
            outs[merge] = out["y"]
        # the same classes, K order and epilogue arithmetic in one launch or four: the same bits
        assert np.array_equal(outs[True], outs[False]), "%s, net %s: merged and per-class outputs differ by %g" % (
            tile, which, float(np.abs(outs[True] - outs[False]).max()))
    # 4: the heads
    case = cases("heads", dtype)
    for fuse in (0, 2):
        outs = {}
        for merge in (True, False):
            out, plan = _run(caffe, case, dtype, fuse, monkeypatch, merge)
            _check_plan(plan, tile, merge and has_mc, _heads_layers(fuse), excused)
            assert sorted(out) == (["prob", "sum1", "sum2"] if fuse == 2 else sorted(k for k in case.ref if k not in case.inputs))
            errs.append(_check_heads(out, case, dtype, fuse, "%s, heads fuse=%d %s" % (tile, fuse, "merged" if merge else "per class")))
            report["merged" if merge and has_mc else "per class"].append("heads/fuse=%d" % fuse)
            outs[merge] = out
        for k in sorted(outs[True]):
            assert np.array_equal(outs[True][k], outs[False][k]), "%s, heads fuse=%d, blob %s: merged and per-class outputs differ by %g" % (
                tile, fuse, k, float(np.abs(outs[True][k] - outs[False][k]).max()))
    print("tile %s (%s): XCD arrangements gx x gy (tiles_m x tiles_n, widths) %s; deconvolutions merged in %s; per class in %s; excused "
          "layers: %s; largest error / range %.3e; largest error / bound so far: %s" % (
              tile, dtype, ", ".join("%s %s" % (n, "off" if not a else "%dx%d (%dx%d, %s)" % a) for n, a in sorted(arr.items())),
              report["merged"] or "-", report["per class"], sorted(excused) or "-", max(errs),
              ", ".join("%s %.3f" % kv for kv in sorted(WORST.items()))))


@pytest.mark.parametrize("v", range(MAX_TILES))
def test_forced_tile_on_small_nets(gpu_caffe, cases, monkeypatch, v):
    table = gpu_caffe.conv_variants()
    if v >= len(table):
        pytest.skip("the variant table has %d entries" % len(table))
    name, esize = table[v]
    monkeypatch.setenv("DC_CONV_VARIANT", str(v))
    _exercise(gpu_caffe, cases, name, "f16" if esize == 2 else "f32", monkeypatch)


@pytest.mark.parametrize("v", range(MAX_TILES_BF16))
def test_forced_bf16_tile_on_small_nets(gpu_caffe, cases, monkeypatch, v):
    table = gpu_caffe.conv_variants_bf16()
    if v >= len(table):
        pytest.skip("the bfloat16 variant table has %d entries" % len(table))
    monkeypatch.setenv("DC_CONV_VARIANT_BF16", str(v))
    _exercise(gpu_caffe, cases, table[v], "bf16", monkeypatch)


def test_tables_are_covered(gpu_caffe):
    names = [n for n, _ in gpu_caffe.conv_variants()]
    bf16 = gpu_caffe.conv_variants_bf16()
    assert 0 < len(names) <= MAX_TILES and 0 < len(bf16) <= MAX_TILES_BF16, "raise MAX_TILES: the tests do not reach the end of a table"
    assert MULTI_CLASS <= set(names) and MULTI_CLASS_BF16 <= set(bf16) and set(EXCUSED) <= set(names) | set(bf16), "a listed tile left the tables"
    assert len(MULTI_CLASS) == 23 and len(MULTI_CLASS_BF16) == 12
    for reason, layers in EXCUSED.values():
        assert reason and layers <= {"dilated", "skip"}
    assert set(XCD_EXCUSED) <= set(names) | set(bf16) and all(XCD_EXCUSED.values())
