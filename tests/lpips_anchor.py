"""An independent float64 anchor of the LPIPS (VGG-16) definition of egogaussian_amd/lpips.py: numpy only, explicit correlation, explicit
floor pooling, an explicit tap list -- nothing of torch's conv2d / max_pool2d, and nothing of the statement's code."""
import numpy as np

MEAN = np.array([-.030, -.088, -.188])
STD = np.array([.458, .448, .450])
# the network as a flat list: ("conv", index) / ("pool",) / ("tap", index) -- the five taps follow relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LAYERS = (("conv", 0), ("conv", 1), ("tap", 0), ("pool",), ("conv", 2), ("conv", 3), ("tap", 1), ("pool",),
          ("conv", 4), ("conv", 5), ("conv", 6), ("tap", 2), ("pool",), ("conv", 7), ("conv", 8), ("conv", 9), ("tap", 3), ("pool",),
          ("conv", 10), ("conv", 11), ("conv", 12), ("tap", 4))


def correlate3x3_relu(f, w, b):
    """f [Cin,H,W], w [Cout,Cin,3,3], b [Cout] -> relu(sum_{c,ky,kx} w[o,c,ky,kx] f0[c, y + ky - 1, x + kx - 1] + b[o]), f0 = f with zeros around."""
    cin, H, W = f.shape
    f0 = np.zeros((cin, H + 2, W + 2))
    f0[:, 1:H + 1, 1:W + 1] = f
    out = np.zeros((w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.tensordot(w[:, :, ky, kx], f0[:, ky:ky + H, kx:kx + W], axes=(1, 0))
    return np.maximum(out + b[:, None, None], 0.0)


def pool2x2_floor(f):
    """The maximum of each whole 2x2 cell; a last odd row / column belongs to no cell."""
    c, H, W = f.shape
    h, w = H // 2, W // 2
    out = np.empty((c, h, w))
    for y in range(h):
        for x in range(w):
            out[:, y, x] = f[:, 2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(c, 4).max(1)
    return out


def taps(v, convs):
    """v [3,H,W] in [0,1]; convs: 13 (w, b) float64 arrays -> the five tap maps [C_k,H_k,W_k]."""
    f = (np.asarray(v, np.float64) - MEAN[:, None, None]) / STD[:, None, None]
    out = []
    for layer in LAYERS:
        if layer[0] == "conv":
            f = correlate3x3_relu(f, *convs[layer[1]])
        elif layer[0] == "pool":
            f = pool2x2_floor(f)
        else:
            out.append(f)
    return out


def lpips(x, y, convs, lins):
    """-> (taps float64[5], their sum)."""
    vals = []
    for fx, fy, l in zip(taps(x, convs), taps(y, convs), lins):
        nx = fx / (np.sqrt((fx * fx).sum(0, keepdims=True)) + 1e-10)
        ny = fy / (np.sqrt((fy * fy).sum(0, keepdims=True)) + 1e-10)
        d = nx - ny
        vals.append(float((l[:, None, None] * d * d).sum(0).sum() / (d.shape[1] * d.shape[2])))
    return np.array(vals), float(sum(vals))


def numpy_weights(weights):
    """egogaussian_amd.lpips.LPIPSWeights -> (convs, lins) as float64 numpy arrays (the float32 values, widened)."""
    return ([(w.double().numpy(), b.double().numpy()) for w, b in weights.convs], [l.double().numpy() for l in weights.lins])
