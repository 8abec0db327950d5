"""Float64 restatements of the 1-D convolutions of csrc/nm_conv.hip (the sentence-CNN encoder's conv + relu + segment
max, the ConvS2S layer's pre-activation) and of their gradients, the slab plan of the weight gradient restated in
Python, and the error bound the direct kernel tests assert.

The bound.  With u = 2^-24 and gamma(K) = K u / (1 - K u), a sum of K fp32 terms added in ANY order, whose products are
exactly rounded or fused, satisfies

    |got - want| <= gamma(K) * mag,

where ``mag`` is the same expression evaluated in float64 on the absolute values of the (fp32-rounded) operands
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; tests/test_imagenet_kernels_gpu.py uses the same
argument for the same MFMA instruction).  K counts every addition the kernels can make on the way to one output:

    pooled forward, width i   w_i E + 1                     window maximum of sum |x||W| + |b|  (max and relu do not
                                                            widen a bound: |max a - max b| <= max |a - b|)
    dx                        sum_i w_i n_i   (+ 1 acc.)    conv^T(|dz|, |W|) (+ |start value|)
                              (the GLU layer adds the residual term dy: one more term, |dy| in mag)
    dW_i                      B S + slices    (+ 1 acc.)    wgrad(|x|, |dz|) (+ |start value|)
    db (pool)                 B S' + 16       (+ 1 acc.)    sum |gated dpooled| (+ |start value|)
    dbias (GLU)               B T + 16        (+ 1 acc.)    column sums of |dz| (+ |start value|)

(the slab sum of conv_wgrad_reduce starts from 0 and adds ``slices`` partial sums; the bias kernels add 16 row lanes).
An absolute floor of K 2^-126 covers flushed denormals.  The operands of the gradient sums are the device's own dz, so
these are pure summation bounds."""
import math

import torch
import torch.nn.functional as TF

U = 2.0 ** -24
TINY = 2.0 ** -126


def gamma(k):
    return k * U / (1.0 - k * U)


def _ref_conv(x, weights, biases):
    """[B, n_i, S] conv1d SAME + b per width, float64 (no relu)."""
    outs = []
    for w, b in zip(weights, biases):
        width = w.shape[0]
        pad = (width - 1) // 2
        xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))
        outs.append(TF.conv1d(xp, w.permute(2, 1, 0)) + b[None, :, None])
    return outs


def _ref_pool(r, s):
    """SAME max-pool of [B, n, S] over windows of s, stride s: [B, n, S']."""
    slen = r.shape[2]
    sp = (slen + s - 1) // s
    pb = (sp * s - slen) // 2
    rp = TF.pad(r, (pb, sp * s - slen - pb), value=-math.inf)
    return rp.view(r.shape[0], r.shape[1], sp, s).max(-1).values


def _ref_conv_t(dz, ws, filters):
    """sum over widths of the transposed convolution of dz [B, S, F]: [B, S, E]."""
    out, col = 0, 0
    for w, (width, n) in zip(ws, filters):
        pad = (width - 1) // 2
        z = dz[:, :, col:col + n].transpose(1, 2)                              # [B, n, S]
        zp = TF.pad(z, (width - 1 - pad, pad))
        out = out + TF.conv1d(zp, w.flip(0).permute(1, 2, 0)).transpose(1, 2)  # weight [E, n, w]
        col += n
    return out


def _ref_wgrad(x, dz, width):
    pad = (width - 1) // 2
    xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))                     # [B, E, S + w - 1]
    slen = x.shape[1]
    return torch.stack([torch.einsum("bes,bsn->en", xp[:, :, k:k + slen], dz) for k in range(width)])


def _pre(x, w, b):
    """tf.nn.conv1d(x, w, 1, "SAME") + b in float64: x [B, T, C], w [width, C, 2C] -> [B, T, 2C]."""
    width = w.shape[0]
    pad = (width - 1) // 2
    xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))
    return TF.conv1d(xp, w.permute(2, 1, 0)).transpose(1, 2) + b


def slab_plan(bsz, slen, e, filters):
    """nm_conv1d_wgrad_workspace_bytes' plan restated (only to name the expected values in the tests): ``tiles`` weight
    gradient tiles of (tap, 64 channels, 64 filters), ``slices`` slabs of ``per`` positions (the last holds ``last``),
    ``slab`` floats each; ``limit`` names what set the slab count."""
    slab = sum(w * e * n for w, n in filters)
    tiles = sum(w * ((e + 63) // 64) * ((n + 63) // 64) for w, n in filters)
    npos = bsz * slen
    limits = {"cap": 32, "positions": npos // 256, "tiles": (2048 + tiles - 1) // tiles}
    limit = min(limits, key=limits.get)                   # (the first of equals)
    slices = max(1, limits[limit])
    per = (npos + slices - 1) // slices
    return dict(tiles=tiles, slices=slices, per=per, last=npos - (slices - 1) * per, slab=slab, limit=limit,
                bytes=slices * slab * 4)


def glu_filters(c, width):
    """The ConvS2S layer as the weight gradient sees it: one width with 2C filters over C channels."""
    return [(width, 2 * c)]


W16 = [(w, 13) for w in list(range(1, 9)) * 2]          # CONV_MAX_WIDTHS filter widths

# case -> ((B, S, E, filters), expected tiles, slices, per, last slab).  The expected values were computed by hand from
# slices = min(ceil(2048 / tiles), (B S) / 256, 32), at least 1; the host tests hold the library to them.
POOL_SLAB_CASES = {
    "P1": ((3, 171, 11, [(2, 13), (4, 200)]), 18, 2, 257, 256),     # two slabs, limited by the positions
    "P2": ((2, 385, 128, [(3, 70), (8, 13)]), 28, 3, 257, 256),     # a seam mid-sentence, two channel / filter tiles
    "P3": ((4, 2000, 11, W16), 72, 29, 276, 272),                   # all 16 widths, limited by the tiles
    "P4": ((8, 1025, 11, [(3, 13)]), 3, 32, 257, 233),              # the cap; the last slab ends in a partial stage
    "P5": ((1, 511, 11, [(3, 13)]), 3, 1, 511, 511),                # just below two slabs
    "P6": ((1, 512, 11, [(3, 13)]), 3, 2, 256, 256),                # just at two slabs
}
GLU_SLAB_CASES = {  # (B, T, C, w)
    "G1": ((2, 257, 13, 5), 5, 2, 257, 257),
    "G2": ((4, 300, 40, 3), 6, 4, 300, 300),                        # slab seams on sentence seams
    "G3": ((3, 260, 72, 8), 48, 3, 260, 260),
}

WORST = {}            # quantity -> the worst err / bound any check of this process saw


def within(got, want, k, mag, what, quantity=None):
    """Assert |got - want| <= gamma(k) mag + k 2^-126 element-wise (k a number or a tensor that broadcasts); prints and
    returns the worst err / bound."""
    k = torch.as_tensor(k, dtype=torch.float64)
    return within_bound(got, want, gamma(k) * mag + k * TINY, what, quantity)


def within_bound(got, want, bound, what, quantity=None):
    """Assert |got - want| <= bound (> 0) element-wise; prints and returns the worst err / bound."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = bound.expand_as(want) if isinstance(bound, torch.Tensor) else torch.full_like(want, bound)
    err = (got - want).abs()
    ok = err <= bound                                                   # a NaN is never within
    ratio = torch.where(ok, err / bound, torch.full_like(err, math.inf))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = quantity or what
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("conv1d bound | {} | {} | worst err / bound {:.4f}".format(key, what, worst))
    assert bool(ok.all()), "{}: {} of {} elements beyond the bound, worst err / bound {:.3f}".format(
        what, int((~ok).sum()), ok.numel(), float((err / bound)[~ok & ~torch.isnan(err)].max())
        if bool((~ok & ~torch.isnan(err)).any()) else math.nan)
    return worst


def bias_shift(window):
    """The bias mean at which about half of the segment maxima of ``window`` unit-variance pre-activations are positive:
    P(max > 0) = 1 - P(one <= 0)^window = 1/2."""
    q = 0.5 ** (1.0 / window)                         # P(pre-activation + shift <= 0)
    return -math.sqrt(2.0) * float(torch.erfinv(torch.tensor(2.0 * q - 1.0, dtype=torch.float64)))


def pool_inputs(bsz, slen, e, filters, s, seed):
    """fp32-rounded x, W_i, b_i (as float64), both signs everywhere; the biases sit where the relu cuts about half of the
    pooled values."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    x = rnd(bsz, slen, e).float().double()
    ws = [(rnd(w, e, n) / math.sqrt(w * e)).float().double() for w, n in filters]
    shift = bias_shift(min(s, slen))
    bs = [(rnd(n) * 0.3 + shift).float().double() for _, n in filters]
    return x, ws, bs, g


def pool_forward_ref(x, ws, bs, s):
    """(pooled [B, S', F], its magnitude [B, S', F], relu(conv) [B, F, S]) in float64."""
    convs = _ref_conv(x, ws, bs)
    mags = _ref_conv(x.abs(), [w.abs() for w in ws], [b.abs() for b in bs])
    ref = torch.cat([_ref_pool(torch.relu(c), s) for c in convs], 1).transpose(1, 2)
    mag = torch.cat([_ref_pool(c, s) for c in mags], 1).transpose(1, 2)
    return ref, mag, torch.relu(torch.cat(convs, 1))


def forward_k(e, filters):
    """K of the pooled forward per output column: w_i E products and the bias."""
    return torch.cat([torch.full((n,), float(w * e + 1), dtype=torch.float64) for w, n in filters])
