"""What a float32 layer is held to: the error of a plain float32 sum.  Plain numpy, for host and GPU tests alike; nothing here uses
the project's library or the C oracle.

  reference   conv_ref64 / deconv_ref64 / epilogue64: float64 throughout, never rounded to float32.
  model       conv_seq32 / deconv_seq32 + epilogue32: the same operation as ONE sequential float32 sum over K in im2col order (input
              channel, kernel row, kernel column), acc = fl(acc + fl(x w)) per element, no FMA, no blocking — the least accurate
              ordering a correct float32 kernel could use; any blocking or split K is more accurate in expectation.
              wino23_f32 / wino43_f32: a Winograd form's own roundings are part of what it is, so its model is a float32 emulation
              of the form (filter transform in double and rounded once as the packers do, input and inverse transform in float32 in
              the kernels' operation order, the per-point products as sequential float32 sums over the input channels).
  statistic   f32_ratios(got, ref64, model32) = (max|got - ref| / max|model - ref|, rms(got - ref) / rms(model - ref)), `got` over
              ALL outputs; the model's statistics over a seeded subset of output pixels (pixel_subset) where M N K > 5e8.
  margins     MARGIN_MAX = 3, MARGIN_RMS = 2 (assert_f32_tight).  Fixed from CPU evidence (tests/test_f32_bound_host.py): correct
              blockings stay at or below 1.1 on both statistics; the margins cover the sample spread of a maximum over 1e4 .. 1e6
              outputs, the unknown internal rounding of the MFMA's own adds and the placement of the affine, and still reject
              operands rounded to 16 significant bits.  They are NOT tuned from what the kernels measure.

Measured on an MI355X, worst over each form's cases (max ratio, RMS ratio):
  form (tests)                                                             cases   max    rms     model
  gather-GEMM tiles, each of the 23 float32 ones forced (test_gpu_tile_shapes)  184   1.13   1.00    sequential sum
  the 26 T2 configurations x batch 1, 2 as lowered (test_gpu_layers)             48   0.78   0.76    sequential sum
    ... the 3x3 rows of them the per-shape timing gave to wino_f23                4   0.70   0.72    wino23_f32
  wino_f23, wino_f23_w16 (test_gpu_winograd)                                     16   1.27   1.00    wino23_f32
  wino_f23_mix, _mix_w16 (test_gpu_winograd_mixed)                               18   1.12   1.00    wino23_f32
  wino_f23_5x6, _5x6_w16 (test_gpu_winograd_blocks)                              22   1.05   1.25    wino23_f32
  wino_f43 (test_gpu_winograd43)                                                 13   1.24   0.87    wino43_f32
  ws1x1f / the tile beside it (test_gpu_stream1x1_f32)                           24   0.79 / 0.82   0.80 / 0.74   sequential sum
  ws7x7f / the row-tap launch beside it (test_gpu_stem_f32)                       8   0.96 / 1.00   0.76 / 1.03   sequential sum
No form needed a rounding the models lack, and none is left on its former bound alone.
"""
import collections
import hashlib

import numpy as np

MARGIN_MAX = 3.0
MARGIN_RMS = 2.0
SUBSET_ABOVE = 5e8   # M N K above which the model may be taken over a subset of the output pixels
SUBSET_MIN = 2048    # the subset's smallest size (all images together)
SUBSET_ENDS = 64     # the first and the last pixels of every image that are always in it
F32 = np.float32


# ---- reference: float64 -------------------------------------------------------------------------------------------------------------
def _out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def conv_ref64(x, w, bias=None, stride=1, pad=0, dilation=1):
    """x [n, cin, h, w], w [cout, cin, k, k] -> float64 [n, cout, oh, ow]: one matrix product per filter tap on a slice of the padded input"""
    n, cin, h, wd = x.shape
    cout, _ci, kh, kw = w.shape
    oh, ow = _out_size(h, kh, stride, pad, dilation), _out_size(wd, kw, stride, pad, dilation)
    xp = np.zeros((n, cin, h + 2 * pad, wd + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    w64 = w.astype(np.float64)
    out = np.zeros((n, cout, oh * ow))
    for ky in range(kh):
        for kx in range(kw):
            y0, x0 = ky * dilation, kx * dilation
            sl = xp[:, :, y0:y0 + stride * (oh - 1) + 1:stride, x0:x0 + stride * (ow - 1) + 1:stride]
            out += np.matmul(w64[:, :, ky, kx], np.ascontiguousarray(sl).reshape(n, cin, oh * ow))
    out = out.reshape(n, cout, oh, ow)
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :, None, None]
    return out


def _deconv_as_conv(x, w, stride, pad, dilation):
    """The transposed convolution y[s iy + d ky - pad] += x[iy] w[ci, co, ky] as a stride-1 convolution: zeros between the input pixels,
    d (k - 1) - pad zeros around them, the filter turned by 180 degrees -> (the spread input, the filter as [cout, cin, k, k], the pad)"""
    n, cin, h, wd = x.shape
    k = w.shape[2]
    up = np.zeros((n, cin, stride * (h - 1) + 1, stride * (wd - 1) + 1), x.dtype)
    up[:, :, ::stride, ::stride] = x
    edge = dilation * (k - 1) - pad
    assert edge >= 0
    return up, np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]), edge


def deconv_ref64(x, w, bias=None, stride=1, pad=0, dilation=1):
    """x [n, cin, h, w], w [cin, cout, k, k] (Caffe's order) -> float64 [n, cout, s (h - 1) + d (k - 1) + 1 - 2 pad, ...]"""
    up, wf, edge = _deconv_as_conv(x, w, stride, pad, dilation)
    return conv_ref64(up, wf, bias, 1, edge, dilation)


def fold_affine64(cout, bias=None, bn=None, scale=None, eps=1e-5):
    """(a, b) of y = a acc + b in float64 from the layer parameters, as fold_bn / fold_scale of csrc/net_lower.cpp fold them:
    bias -> (1, bias); BatchNorm (mean, var, scale factor) -> s = 1 / sqrt(var / sf + eps), a *= s, b = (b - mean / sf) s;
    Scale (gamma, beta) -> a *= gamma, b = b gamma + beta.  (None, None) without any of them."""
    if bias is None and bn is None and scale is None:
        return None, None
    a, b = np.ones(cout), np.zeros(cout)
    if bias is not None:
        b = np.asarray(bias, F32).astype(np.float64)
    if bn is not None:
        mean, var, sf = [np.asarray(v, F32).astype(np.float64) for v in bn]
        sf = 0.0 if float(sf.ravel()[0]) == 0.0 else 1.0 / float(sf.ravel()[0])
        s = 1.0 / np.sqrt(var * sf + eps)
        a, b = a * s, (b - mean * sf) * s
    if scale is not None:
        g = np.asarray(scale[0], F32).astype(np.float64)
        a, b = a * g, b * g
        if len(scale) > 1 and scale[1] is not None:
            b = b + np.asarray(scale[1], F32).astype(np.float64)
    return a, b


def fold_layers64(cout, weights):
    """fold_affine64 from a test's weight list [(name, type, blobs)]: the Convolution's bias, a BatchNorm, a Scale"""
    bias = bn = scale = None
    for _name, typ, blobs in weights:
        if typ in ("Convolution", "Deconvolution") and len(blobs) > 1:
            bias = blobs[1]
        elif typ == "BatchNorm":
            bn = blobs
        elif typ == "Scale":
            scale = blobs
    return fold_affine64(cout, bias, bn, scale)


def _per_channel(v, like):
    return np.asarray(v).reshape((1, -1) + (1,) * (like.ndim - 2))


def epilogue64(acc, a=None, b=None, shortcut=None, relu=False):
    """a acc + b per channel (axis 1), + shortcut, ReLU: float64"""
    y = np.asarray(acc, np.float64)
    if a is not None:
        y = y * _per_channel(a, y) + _per_channel(b, y)
    if shortcut is not None:
        y = y + np.asarray(shortcut, np.float64)
    return np.maximum(y, 0.0) if relu else y


def epilogue32(acc, a=None, b=None, shortcut=None, relu=False):
    """fl(fl(acc a32) + b32), then + shortcut, then ReLU, each in float32 (a, b: the float64 fold rounded once, as the device gets them)"""
    y = np.asarray(acc, F32)
    if a is not None:
        y = y * _per_channel(a, y).astype(F32)
        y = y + _per_channel(b, y).astype(F32)
    if shortcut is not None:
        y = y + np.asarray(shortcut, F32)
    return np.maximum(y, F32(0)) if relu else y


# ---- float32 products ---------------------------------------------------------------------------------------------------------------
_BLOCK = 1 << 15  # output elements per block of the loops below: two float32 blocks stay in a core's cache


def seq_dot32(A, B):
    """A [M, K] B[N, K]^T in float32 as one sequential sum per output: acc = fl(acc + fl(a_k b_k)), k ascending"""
    return blocked_dot32(A, B, 1)


def blocked_dot32(A, B, chunk=1, split=1):
    """A [M, K] B[N, K]^T in float32 the way a blocked kernel sums it.  chunk = 1: fl(a_k b_k) added one by one.  chunk = c > 1: the c
    products of a chunk summed exactly (float64) and rounded once — one matrix instruction —, the chunk sums added one by one in float32.
    split = s: K dealt into s contiguous runs of whole chunks, each summed as above from zero, the s partial sums added in float32 in
    order (split K)."""
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    (M, K), N = A.shape, B.shape[0]
    assert B.shape[1] == K
    nch = -(-K // chunk)
    if nch * chunk != K:  # whole chunks: zero products change no sum
        A = np.concatenate([A, np.zeros((M, nch * chunk - K), F32)], 1)
        B = np.concatenate([B, np.zeros((N, nch * chunk - K), F32)], 1)
    Bt = np.ascontiguousarray(B.T) if chunk == 1 else np.ascontiguousarray(B.T, np.float64)
    runs = [(nch * s // split, nch * (s + 1) // split) for s in range(split)]
    out = np.empty((M, N), F32)
    rows = max(1, _BLOCK // N)
    for m0 in range(0, M, rows):
        a = A[m0:m0 + rows] if chunk == 1 else A[m0:m0 + rows].astype(np.float64)
        total = None
        tmp = np.empty((a.shape[0], N), F32)
        for c0, c1 in runs:
            acc = np.zeros((a.shape[0], N), F32)
            for c in range(c0, c1):
                if chunk == 1:
                    np.multiply(a[:, c, None], Bt[c][None, :], out=tmp)
                    acc += tmp
                else:
                    acc += np.matmul(a[:, c * chunk:(c + 1) * chunk], Bt[c * chunk:(c + 1) * chunk]).astype(F32)
            total = acc if total is None else total + acc
        out[m0:m0 + rows] = total
    return out


def round_bits(a, bits):
    """a (float32) rounded to `bits` significant bits, ties to even: 24 is float32 itself, 16 a bf16 hi + lo pair, 11 float16 / tf32"""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits).astype(F32)


# ---- model: one sequential float32 sum ----------------------------------------------------------------------------------------------
def pixel_subset(n, npix, cout, K):
    """None (every pixel) where M N K = n npix cout K <= 5e8, else the sorted pixel indices (the same in every image) the model is
    taken over: about 5e8 / (N K) pixels in all and never fewer than 2048, the first 64 and the last 64 of an image always among them,
    the rest drawn with a fixed seed"""
    if float(n) * npix * cout * K <= SUBSET_ABOVE:
        return None
    per = -(-max(SUBSET_MIN, int(SUBSET_ABOVE // (cout * K))) // n)
    if per >= npix:
        return None
    ends = np.r_[0:min(SUBSET_ENDS, npix), max(0, npix - SUBSET_ENDS):npix]
    rest = np.setdiff1d(np.arange(npix), ends)
    more = np.random.RandomState(2024).choice(rest, max(0, per - len(np.unique(ends))), replace=False)
    return np.unique(np.r_[ends, more])


def im2col32(x, k, stride=1, pad=0, dilation=1, pixels=None):
    """x [n, cin, h, w] -> float32 [n, pixels, cin k k]: K in im2col order (input channel, kernel row, kernel column)"""
    n, cin, h, wd = x.shape
    oh, ow = _out_size(h, k, stride, pad, dilation), _out_size(wd, k, stride, pad, dilation)
    xp = np.zeros((n, cin, h + 2 * pad, wd + 2 * pad), F32)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    npix = oh * ow if pixels is None else len(pixels)
    cols = np.empty((n, npix, cin, k, k), F32)
    for ky in range(k):
        for kx in range(k):
            y0, x0 = ky * dilation, kx * dilation
            sl = xp[:, :, y0:y0 + stride * (oh - 1) + 1:stride, x0:x0 + stride * (ow - 1) + 1:stride].reshape(n, cin, oh * ow)
            cols[:, :, :, ky, kx] = (sl if pixels is None else sl[:, :, pixels]).transpose(0, 2, 1)
    return cols


def _conv32(x, wmat, k, stride, pad, dilation, pixels, dot, flip=False):
    cols = im2col32(x, k, stride, pad, dilation, pixels)
    n, npix = cols.shape[:2]
    if flip:  # a deconvolution's K runs over ITS kernel rows and columns, not the turned filter's
        cols = cols[:, :, :, ::-1, ::-1]
    out = dot(cols.reshape(n * npix, -1), wmat)  # [n pixels, cout]
    return np.ascontiguousarray(out.reshape(n, npix, -1).transpose(0, 2, 1))


def conv_seq32(x, w, stride=1, pad=0, dilation=1, pixels=None, dot=seq_dot32):
    """The convolution's sums as the model takes them -> float32 [n, cout, oh ow] (or [n, cout, len(pixels)]); epilogue32 goes on top.
    `dot` replaces the sequential product (tests/test_f32_bound_host.py: blocked and wrong models)."""
    cout, _cin, k, _k = w.shape
    return _conv32(np.asarray(x, F32), np.asarray(w, F32).reshape(cout, -1), k, stride, pad, dilation, pixels, dot)


def deconv_seq32(x, w, stride=1, pad=0, dilation=1, pixels=None, dot=seq_dot32):
    """The transposed convolution likewise (w [cin, cout, k, k]); taps that fall between the input pixels are zero products, which
    change no float32 sum"""
    up, wf, edge = _deconv_as_conv(np.asarray(x, F32), np.asarray(w, F32), stride, pad, dilation)
    k = w.shape[2]
    wmat = np.ascontiguousarray(wf[:, :, ::-1, ::-1]).reshape(wf.shape[0], -1)
    return _conv32(up, wmat, k, 1, edge, dilation, pixels, dot, flip=True)


# ---- models: the Winograd forms in float32 ------------------------------------------------------------------------------------------
G23 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
G43 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)


def _phase_patches(x, d, m, T):
    """The (m + 2)^2 pixel planes of every tile of F(m x m, 3x3) on the dilation-phase images of x: [m + 2][m + 2] arrays [R, cin], rows
    r = ((n d d + phase) TY + ty) TX + tx; every phase image gets the same TY x TX grid, pixels outside an image are zeros (ragged last
    tiles, the smaller phases' surplus tiles)"""
    n, cin, h, w = x.shape
    TY, TX = T
    planes = [[[] for _ in range(m + 2)] for _ in range(m + 2)]
    for img in range(n):
        for py in range(d):
            for px in range(d):
                ph = x[img, :, py::d, px::d]
                pad = np.zeros((cin, m * TY + 2, m * TX + 2), F32)
                pad[:, 1:1 + ph.shape[1], 1:1 + ph.shape[2]] = ph
                for a in range(m + 2):
                    for b in range(m + 2):
                        planes[a][b].append(pad[:, a:a + m * TY:m, b:b + m * TX:m].reshape(cin, TY * TX).T)
    return [[np.concatenate(planes[a][b], 0) for b in range(m + 2)] for a in range(m + 2)]


def _scatter_tiles(Y, n, cout, h, w, d, m, T):
    """Y[a][b] [R, cout] -> [n, cout, h, w]: output pixel (a, b) of every tile back onto the phase images, pixels past an image dropped"""
    TY, TX = T
    out = np.zeros((n, cout, h, w), F32)
    r = 0
    for img in range(n):
        for py in range(d):
            for px in range(d):
                dst = out[img, :, py::d, px::d]
                full = np.zeros((cout, m * TY, m * TX), F32)
                for a in range(m):
                    for b in range(m):
                        full[:, a::m, b::m] = Y[a][b][r:r + TY * TX].T.reshape(cout, TY, TX)
                dst[...] = full[:, :dst.shape[1], :dst.shape[2]]
                r += TY * TX
    return out


def _bt23(d):  # csrc/wino_f32.hip: i = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3 (one float32 add each)
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def _at23(m):  # ... the inverse: m0 + m1 + m2, m1 - m2 - m3, left to right
    return [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]


def wino23_f32(x, g, d=1, dot=seq_dot32, vround=None):
    """Winograd F(2x2, 3x3) as wino_f23_kernel (csrc/wino_f32.hip) computes a pad = dilation = d 3x3 layer, every stage in float32 ->
    [n, cout, h, w] before the epilogue.  U = G g G^T in double, rounded once (wino_pack_filters); V = B^T d B on the 4 x 4 patches of
    the d x d phase images, along the patch rows first, then along the columns, one add per entry and stage; 16 products M[i][j] = V[i][j]
    U[i][j]^T over the input channels (`dot`; the kernel's chains of four and, with 16 waves, two groups are blockings of it); Y = A^T M A
    over j, then over i.  Block geometry and wave count do not enter: a tile's arithmetic does not depend on the slot it sits in.
    `vround` is applied to V (tests/test_f32_bound_host.py: a transform at reduced precision)."""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    n, cin, h, w = x.shape
    cout = g.shape[0]
    T = ((-(-h // d) + 1) // 2, (-(-w // d) + 1) // 2)
    U = np.einsum("ia,ocab,jb->ijoc", G23, g.astype(np.float64), G23).astype(F32)
    P = _phase_patches(x, d, 2, T)
    t = [_bt23([P[a][b] for a in range(4)]) for b in range(4)]       # t[b][i]: along the patch rows
    V = [_bt23([t[b][i] for b in range(4)]) for i in range(4)]       # V[i][j]: along the columns
    if vround is not None:
        V = [[vround(v) for v in row] for row in V]
    M = [[dot(V[i][j], U[i, j]) for j in range(4)] for i in range(4)]
    Pj = [_at23(M[i]) for i in range(4)]                              # Pj[i][b]
    Y = [[_at23([Pj[i][b] for i in range(4)])[a] for b in range(2)] for a in range(2)]
    return _scatter_tiles(Y, n, cout, h, w, d, 2, T)


def _bt43(d):  # w43_bt of csrc/wino43_f32.hip, operation for operation (products by 4 and 2 are exact, by 5 rounded)
    o0 = (F32(4) * d[0] - F32(5) * d[2]) + d[4]
    s0, s1 = d[4] - F32(4) * d[2], d[3] - F32(4) * d[1]
    s2, s3 = d[4] - d[2], F32(2) * (d[3] - d[1])
    return [o0, s0 + s1, s0 - s1, s2 + s3, s2 - s3, (F32(4) * d[1] - F32(5) * d[3]) + d[5]]


def _at43(m):  # w43_at
    a0, a1, b0, b1 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return [(m[0] + a0) + b0, a1 + F32(2) * b1, a0 + F32(4) * b0, (a1 + F32(8) * b1) + m[5]]


def wino43_f32(x, g, d=1, dot=seq_dot32, vround=None):
    """Winograd F(4x4, 3x3) as the three kernels of the unfused form compute it (csrc/wino43_f32.hip), every stage in float32 ->
    [n, cout, h, w] before the epilogue.  U = G g G^T in double, rounded once (dc_wino43_pack); V = B^T d B per 6 x 6 patch on the
    dilation-phase tile grid, along the rows, then the columns (w43_bt); 36 products M[p] = V[p] U[p]^T (`dot`); Y = A^T M A, columns
    first (w43_at)."""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    n, cin, h, w = x.shape
    cout = g.shape[0]
    T = ((-(-h // d) + 3) // 4, (-(-w // d) + 3) // 4)
    U = np.einsum("ia,ocab,jb->ijoc", G43, g.astype(np.float64), G43).astype(F32)
    P = _phase_patches(x, d, 4, T)
    v = [_bt43(P[i]) for i in range(6)]                                # v[i][j]: d B, along the row
    V = [[None] * 6 for _ in range(6)]
    for j in range(6):
        col = _bt43([v[i][j] for i in range(6)])                       # B^T (d B), along the column
        for i in range(6):
            V[i][j] = col[i]
    if vround is not None:
        V = [[vround(e) for e in row] for row in V]
    M = [[dot(V[i][j], U[i, j]) for j in range(6)] for i in range(6)]
    W = [[None] * 6 for _ in range(4)]
    for j in range(6):
        col = _at43([M[i][j] for i in range(6)])                       # A^T M
        for i in range(4):
            W[i][j] = col[i]
    Y = [_at43(W[i]) for i in range(4)]
    return _scatter_tiles(Y, n, cout, h, w, d, 4, T)


# ---- statistic ----------------------------------------------------------------------------------------------------------------------
def _flat(a):
    return np.asarray(a).reshape(a.shape[0], a.shape[1], -1)


def _stats(got, ref64, model32, pixels):
    got, ref = _flat(got), _flat(ref64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rsub = ref if pixels is None else ref[:, :, pixels]
    model = _flat(model32)
    assert model.shape == rsub.shape, (model.shape, rsub.shape)
    eg, em = got.astype(np.float64) - ref, model.astype(np.float64) - rsub
    return float(np.abs(eg).max()), float(np.abs(em).max()), float(np.sqrt(np.mean(eg * eg))), float(np.sqrt(np.mean(em * em)))


def f32_ratios(got, ref64, model32, pixels=None):
    """(max|got - ref| / max|model - ref|, rms(got - ref) / rms(model - ref)): `got` and `ref64` [n, c, ...] over all outputs, `model32`
    over all of them or, with `pixels` (pixel_subset), [n, c, len(pixels)] over those"""
    gmax, mmax, grms, mrms = _stats(got, ref64, model32, pixels)
    return gmax / mmax, grms / mrms


WORST = {}  # label prefix (up to the first ':') -> [largest max ratio, largest rms ratio] seen in this process


def assert_f32_tight(got, ref64, model32, label, pixels=None):
    """Both ratios within the margins; the figures are printed (shown under -s, and with a failure)"""
    gmax, mmax, grms, mrms = _stats(got, ref64, model32, pixels)
    rmax, rrms = gmax / mmax, grms / mrms
    w = WORST.setdefault(label.split(":")[0], [0.0, 0.0])
    w[0], w[1] = max(w[0], rmax), max(w[1], rrms)
    print("f32 %s: max %.3e / model %.3e = %.2f (<= %g), rms %.3e / model %.3e = %.2f (<= %g); worst so far %.2f, %.2f" % (
        label, gmax, mmax, rmax, MARGIN_MAX, grms, mrms, rrms, MARGIN_RMS, w[0], w[1]))
    assert rmax <= MARGIN_MAX and rrms <= MARGIN_RMS, "%s: max error %.3e is %.2f x the sequential float32 model's %.3e (margin %g), rms %.3e is %.2f x its %.3e (margin %g)" % (
        label, gmax, rmax, mmax, MARGIN_MAX, grms, rrms, mrms, MARGIN_RMS)
    return rmax, rrms


# ---- one layer of a test: reference and model, made once ---------------------------------------------------------------------------
_memo = collections.OrderedDict()
_MEMO_KEEP = 16  # layers kept: more than the nets of a forced-tile sweep or the cases of one Winograd file, whose runs come back to a layer


def _key(*parts):
    h = hashlib.sha1()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()


class Layer(object):
    """One layer of a test: .ref64 (float64, all outputs), .model32 (the sequential model, over .pixels where that is not None);
    unpacks as (ref64, model32, pixels).  .model(dot) is the same layer with another product in the model's place, over the same pixels."""

    def __init__(self, kind, x, w, a, b, shortcut, relu, stride, pad, dilation):
        self.args = (kind, x, w, a, b, shortcut, relu, stride, pad, dilation)
        deconv = kind == "deconv"
        acc64 = (deconv_ref64 if deconv else conv_ref64)(x, w, None, stride, pad, dilation)
        cout, K = w.shape[1 if deconv else 0], w.shape[0 if deconv else 1] * w.shape[2] * w.shape[3]
        self.pixels = pixel_subset(acc64.shape[0], acc64.shape[2] * acc64.shape[3], cout, K) if kind in ("conv", "deconv") else None
        sc = None if shortcut is None else _flat(shortcut)
        self.ref64 = epilogue64(_flat(acc64), a, b, sc, relu).reshape(acc64.shape)
        self.model32 = self.model(seq_dot32)
        self.ref64.setflags(write=False)
        self.model32.setflags(write=False)

    def model(self, dot):
        kind, x, w, a, b, shortcut, relu, stride, pad, dilation = self.args
        if kind == "conv":
            acc32 = conv_seq32(x, w, stride, pad, dilation, self.pixels, dot)
        elif kind == "deconv":
            acc32 = deconv_seq32(x, w, stride, pad, dilation, self.pixels, dot)
        else:
            assert kind in ("wino23", "wino43") and stride == 1 and pad == dilation and w.shape[2] == 3, kind
            acc32 = _flat((wino23_f32 if kind == "wino23" else wino43_f32)(x, w, dilation, dot))
        sc = None if shortcut is None else _flat(shortcut)
        return epilogue32(acc32, a, b, sc if sc is None or self.pixels is None else sc[:, :, self.pixels], relu)

    def ref_on_pixels(self):
        r = _flat(self.ref64)
        return r if self.pixels is None else r[:, :, self.pixels]

    def __iter__(self):
        return iter((self.ref64, self.model32, self.pixels))


def layer_case(kind, x, w, a=None, b=None, shortcut=None, relu=False, stride=1, pad=0, dilation=1):
    """The Layer of one layer with its epilogue, made once per input and kept while recently used (keyed by content: the forms of one layer, the forced tiles of a
    sweep and test modules with the same seeded data share it) and left unchanged.  kind: "conv" / "deconv" (the sequential model),
    "wino23" / "wino43" (the form's emulation; stride 1, pad = dilation)."""
    key = _key(kind, x, w, a, b, shortcut, relu, stride, pad, dilation)
    if key not in _memo:
        _memo[key] = Layer(kind, x, w, a, b, shortcut, relu, stride, pad, dilation)
        while len(_memo) > _MEMO_KEEP:
            _memo.popitem(last=False)
    _memo.move_to_end(key)
    return _memo[key]
