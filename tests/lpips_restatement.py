"""The LPIPS rules (include/hive_mi355x.h, above hive_lpips_create) stated literally: the input table in numpy, the five feature rows in torch on the CPU in
float64 through conv2d and max_pool2d, the tail in numpy float64 in the stated order with math.fsum for the means; beside it the whole score in float32 torch-CPU
operators as the lpips package arranges them (the reference's arithmetic), and the feature rows on integer-valued data for the exact tests.  lpips and torchvision
are absent: the network is lpips.LPIPS(net='alex'), version 0.1, eval mode, from its published definition.  What csrc/lpips.hip must reproduce: integer-valued
feature rows and the distance maps bit for bit, real-valued rows within the float32 summation bound, scores within a stated distance.  numpy's element-wise float64
operators round once per operation (no fused multiply-add), like the kernels' build.  Imports nothing from the package.

`weights` everywhere: an object with conv_w[l] (O, I, k, k), conv_b[l] (O,) and lin_w[l] (O,), float32 numpy arrays."""
import math

import numpy as np

# (C_in, C_out, kernel, stride, padding, a maxpool 3 / 2 in front)
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
U = 2.0 ** -24  # the unit roundoff of float32


def input_table():
    """float32 (3, 256): the value of a byte, ((v / 255) * 2.0 - 1.0) in float64 rounded to float32, then the scaling layer (x - shift[k]) / scale[k] in float32."""
    v = np.arange(256, dtype=np.float64)
    x = ((v / 255) * 2.0 - 1.0).astype(np.float32)
    return np.stack([(x - np.float32(SHIFT[k])) / np.float32(SCALE[k]) for k in range(3)])


def scaled_input(image):
    """uint8 (..., 3) -> float32 (..., 3): channel k of the picture through row k of the table."""
    image = np.asarray(image)
    table = input_table()
    return np.stack([table[k][image[..., k]] for k in range(3)], -1)


def mask_background(ref, est):
    """masked_frame[color_np == [255, 255, 255]] = 255: per channel (the rule of similarity_restatement.mask_background)."""
    out = np.array(ref, copy=True)
    out[np.asarray(est) == [255, 255, 255]] = 255
    return out


def feature_sizes(h, w):
    sizes = []
    for _, _, k, stride, pad, pool in LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        sizes.append((h, w))
    return sizes


def _pre_activation(index, x, w, b):
    """x torch (N, C_in, h, w) -> the convolution with bias of row `index`, after its pool, in x's dtype."""
    import torch.nn.functional as F
    _, _, _, stride, pad, pool = LAYERS[index]
    if pool:
        x = F.max_pool2d(x, kernel_size=3, stride=2)
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def layer(index, x, weights, dtype=np.float64):
    """One feature row: x (N, h, w, C_in) channels last, the previous row's ReLU map un-pooled -> (N, ho, wo, C_out), computed in `dtype` on the CPU."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype)))
    y = torch.relu(_pre_activation(index, t(x).permute(0, 3, 1, 2), t(weights.conv_w[index]), t(weights.conv_b[index])))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def _magnitude(index, x, weights):
    """sum |w| |x| + |b| per output value, float64 (N, ho, wo, C_out)."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.abs(np.asarray(a, dtype=np.float64))))
    mag = _pre_activation(index, t(x).permute(0, 3, 1, 2), t(weights.conv_w[index]), t(weights.conv_b[index]))
    return mag.permute(0, 2, 3, 1).contiguous().numpy()


def layer_bound(index, x, weights):
    """gamma_K (sum |w| |x| + |b|) per output value: what a float32 sum of the row's K products and its bias, in ANY order, may differ by from exact
    arithmetic.  K counts the products and the bias."""
    cin, _, k, _, _, _ = LAYERS[index]
    K = cin * k * k + 1
    return (K * U / (1 - K * U)) * _magnitude(index, x, weights)


def layer_int(index, x, weights):
    """The row on integer-valued data, exactly: every partial sum stays below 2^24 (checked), so float64 holds it and float32 does in any order -> float32."""
    for a in (x, weights.conv_w[index], weights.conv_b[index]):
        assert np.array_equal(a, np.rint(a)), "integer-valued data only"
    largest = float(_magnitude(index, x, weights).max())
    assert largest < 2 ** 24, largest
    out = layer(index, x, weights, np.float64)
    assert np.array_equal(out, np.rint(out))
    return out.astype(np.float32)


def features(image, weights, dtype=np.float64):
    """The five ReLU maps of uint8 pictures (N, H, W, 3), each (N, h_l, w_l, C_l), every row computed in `dtype` from the row before."""
    x = scaled_input(image)
    maps = []
    for index in range(5):
        x = layer(index, x, weights, dtype)
        maps.append(x)
    return maps


def distance_map(a, b, lin_w):
    """The tail of one layer from float32 maps a, b (..., C) -> float64 (...): c ascending, every sum left to right from 0.0."""
    a, b, w = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(lin_w, dtype=np.float64)
    sa, sb = np.zeros(a.shape[:-1]), np.zeros(a.shape[:-1])
    for c in range(a.shape[-1]):
        sa = sa + a[..., c] * a[..., c]
        sb = sb + b[..., c] * b[..., c]
    na, nb = np.sqrt(sa) + 1e-10, np.sqrt(sb) + 1e-10
    d = np.zeros(a.shape[:-1])
    for c in range(a.shape[-1]):
        t = a[..., c] / na - b[..., c] / nb
        d = d + w[c] * (t * t)
    return d


def layer_score(d):
    """The spatial mean of one picture's map, summed without error."""
    return math.fsum(np.asarray(d).ravel()) / d.size


def score_from_features(maps_ref, maps_est, weights, picture=0):
    """(the score, the five layer scores, the five maps) of one picture from float32 feature maps: the tail alone."""
    dists = [distance_map(maps_ref[l][picture], maps_est[l][picture], weights.lin_w[l]) for l in range(5)]
    layers = [layer_score(d) for d in dists]
    total = layers[0]
    for value in layers[1:]:
        total = total + value
    return total, layers, dists


def score(ref, est, weights):
    """The restatement's LPIPS of one uint8 (H, W, 3) pair: float64 features, the float64 tail -> (score, [five layer scores])."""
    fa, fb = features(np.asarray(ref)[None], weights), features(np.asarray(est)[None], weights)
    total, layers, _ = score_from_features(fa, fb, weights)
    return total, layers


def score_f32(ref, est, weights):
    """The same pair through float32 torch-CPU operators arranged as the lpips package arranges them (normalize_tensor, the squared difference, the 1 x 1
    linear layer, the spatial average, the sum over the layers): the reference's arithmetic -> (score, [five layer scores]) as Python floats."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))

    def maps(image):
        x = t(scaled_input(np.asarray(image)[None])).permute(0, 3, 1, 2)
        out = []
        for index in range(5):
            x = torch.relu(_pre_activation(index, x, t(weights.conv_w[index]), t(weights.conv_b[index])))
            out.append(x)
        return out

    def normalize(x, eps=1e-10):
        return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)

    fa, fb = maps(ref), maps(est)
    layers = []
    for l in range(5):
        diff = (normalize(fa[l]) - normalize(fb[l])) ** 2
        layers.append(F.conv2d(diff, t(weights.lin_w[l]).reshape(1, -1, 1, 1)).mean([2, 3], keepdim=True))
    total = layers[0]
    for value in layers[1:]:
        total = total + value
    return float(total), [float(v) for v in layers]
