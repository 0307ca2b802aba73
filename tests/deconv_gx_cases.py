"""Shared helpers of the tests of Conv3DTranspose on the 16-bit / split-half graph executor
(test_gpu_deconv_gx.py, test_deconv_gx_host.py; tools/bench_configs.py --what deconv).

`unet_t3` is the smallest U-Net with a learned up-convolution that csrc/gx_exec.h takes whole: the
concatenation is read by a 3x3x3 convolution (tests/deconv_cases.tiny_unet_t reads it with a 1x1x1
one, which the executor declines).  `layer_alone` puts one deconv of a given width class and epilogue
where the executor's output shows it.  The float64 restatement is deconv_cases.graph_forward64.
"""
import numpy as np

from flypylib_amd.program import LayerGraph
from oracle import infer_oracle
from tests import deconv_cases as dc


def unet_t3(in_sz=None, seed=3):
    """conv3(1->16) BN ReLU [T-2] | pool | conv3(16->32) BN ReLU [(T-2)/2-2] | deconv(32->16, bias)
    BN ReLU [T-6] | concat with crop(c1, 2) | conv3(32->16) BN ReLU [T-8] | conv1(16->1, bias, sigmoid).

    rf_info, derived: the three 3x3x3 convolutions see 1 + 2 + 2 * 2 + 2 = 9 input voxels per axis (the
    second one works at half resolution), the up-convolution and the head add none: rf_size 9,
    rf_offset 4; one output per input voxel inside the offset: rf_stride 1."""
    in_sz = (24, 24, 24) if in_sz is None else in_sz
    g = LayerGraph(in_sz, seed=seed)
    c1 = g.conv_bn_relu(g.input(), 16, 3)
    c2 = g.conv_bn_relu(g.pool(c1), 32, 3)
    u = g.bn_relu(g.deconv(c2, 16, use_bias=True))
    m = g.concat(u, g.crop(c1, 2))
    h = g.conv_bn_relu(m, 16, 3)
    g.finish(g.conv(h, 1, 1, use_bias=True, activation='sigmoid'))
    return g, (9, 4, 1), in_sz, None


def unet_t3_random(in_sz=None):
    g, rf, sz, ca = unet_t3(in_sz)
    return dc.randomize(g), rf, sz, ca


EPILOGUES = ('relu', 'bn_relu', 'add')


def tile_of(cin, edge=5):
    """layer_alone's tile for a deconv input of `edge`^3 voxels"""
    return 2 * (edge + (2 if cin > 96 else 0)) + 2


def layer_alone(cin, cout, bias, epilogue, edge=5, seed=0):
    """first layer -> pool -> [conv1 to `cin` channels] -> deconv(cin -> cout) -> ... -> head, for a
    deconv input of `edge`^3 voxels (tile: tile_of; the pool is there so that the network has one
    output per input voxel; 128 channels come from a 3x3x3 convolution); returns (graph, rf_offset).

    'relu': ReLU on the layer, then the head (offset 1).  'bn_relu': folded BN + ReLU, then a 3x3x3
    convolution and the head (offset 2).  'add': no activation, added to a 1x1x1 convolution (ReLU)
    of itself - an activation in front of the Add, so the stand-alone Add kernel runs -, ReLU, head
    (offset 1)."""
    assert epilogue in EPILOGUES
    T = tile_of(cin, edge)
    g = LayerGraph((T,) * 3, seed=seed)
    x = g.pool(g.conv_bn_relu(g.input(), min(cin, 32), 3))
    if cin > 96:                     # (the executor's 1x1x1 convolutions have up to 96 outputs, its 3x3x3 ones 128)
        x = g.conv_bn_relu(x, cin, 3)
    elif cin > 32:
        x = g.conv_bn_relu(x, cin, 1)
    if epilogue == 'relu':
        y, off = g.deconv(x, cout, use_bias=bool(bias), activation='relu'), 1
    elif epilogue == 'bn_relu':
        y = g.bn_relu(g.deconv(x, cout, use_bias=bool(bias)))
        y, off = g.conv_bn_relu(y, 16, 3), 2
    else:
        d = g.deconv(x, cout, use_bias=bool(bias))
        y, off = g.relu(g.add(g.conv_bn_relu(d, cout, 1), d)), 1
    g.finish(g.conv(y, 1, 1, use_bias=True, activation='sigmoid'))
    if cin > 96:
        off += 2                     # the 3x3x3 convolution at half resolution
    return dc.randomize(g, seed + 1), off


def lattice_oracle(g, img, tile, off):
    """float64 graph walk over the reference's tile lattice (as test_gpu_graph_split._oracle)"""
    def f64(batch):
        return dc.graph_forward64(g, batch.astype(np.float64))
    return infer_oracle.infer_lattice(img, (tile,) * 3, (off,) * 3, f64)
