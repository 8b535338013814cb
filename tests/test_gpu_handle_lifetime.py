"""What a pipeline handle holds on the device — buffers, streams, events — goes back when it is closed or its creation is refused.

Every handle's device resources are created and released by one owner (csrc/mpn_internal.h DeviceOwner); the debug
flavour of the library counts what all owners of the process hold (mpn_debug_live_resources).  The tests run on that flavour and compare
DELTAS of the count around the code under test (session fixtures of other modules may hold handles), closing every handle explicitly."""
import ctypes as C

import numpy as np
import pytest
import torch

from multipathnet_amd import _lib, models

pytestmark = pytest.mark.gpu

PLAIN_CFG = [8, 8, "P", 16, "P", 16]                                  # test_gpu_pipeline.py's smallest trunk: 4 conv layers
MPN_CFG = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]


def _live(lib):
    """(buffers, streams, events) held by the owners of the debug library right now"""
    b, s, e = C.c_long(), C.c_long(), C.c_long()
    lib.mpn_debug_live_resources.restype = None
    lib.mpn_debug_live_resources(C.byref(b), C.byref(s), C.byref(e))
    return b.value, s.value, e.value


def _boxes(rng, n, W, H, lo=8):
    c = rng.uniform([1, 1], [W, H], (n, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(min(W, H)), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(np.float32)


def _inputs(dev, H, W, n, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).to(dev), torch.from_numpy(_boxes(rng, n, W, H)).to(dev)


def _plain(**kw):
    P = models.synthetic_params(PLAIN_CFG, pooled=7, fc_dim=32, n_classes=4, seed=1)
    return models.FastRCNN(P, cfg=PLAIN_CFG, pooled=7, spatial_scale=0.25, max_h=150, max_w=256, max_rois=64, **kw)


def _mpnet(fc_dim, **kw):
    P = models.synthetic_mpnet_params(MPN_CFG, pooled=7, fc_dim=fc_dim, n_classes=9, n_integral=3, seed=11)
    return models.MultiPathNet(P, cfg=MPN_CFG, pooled=7, spatial_scale=1 / 16, max_h=150, max_w=250, max_rois=120, **kw)


@pytest.mark.parametrize("kind", ["rbox_scores_one_pass", "mpnet_fc_dim_32"])
def test_refused_create_holds_nothing(dev, kind):
    """Configurations that are refused only late in create (use_rbox_scores needs two passes; MultiPathNet's fc_dim must be a multiple of
    128) once kept the trunk, head and tail they had allocated by then."""
    with _lib.debug_hooks() as lib:
        before = _live(lib)
        with pytest.raises(_lib.MpnError):
            if kind == "rbox_scores_one_pass":
                _plain(use_rbox_scores=True, num_iter=1)
            else:
                _mpnet(32)
        torch.cuda.synchronize()
        assert _live(lib) == before


def test_plain_handle_returns_everything(dev):
    """create -> every entry point that makes the handle allocate, create a stream or an event -> close"""
    with _lib.debug_hooks() as lib:
        start = _live(lib)
        net = _plain()
        assert _live(lib)[0] - start[0] >= 4                          # at least the conv layers' buffers: the counter moves
        im, bx = _inputs(dev, 150, 256, 64)
        net.detect(im, bx)
        for _ in range(3):                                            # deferred heads: y7 / boxes copies, ev_fc7
            net.test_one_pipelined(im, bx)
        pin = [(im.cpu().pin_memory(), bx.cpu().pin_memory()) for _ in range(2)]
        for i in range(4):                                            # copy stream, staging sets (all three of them)
            net.test_one_pipelined_host(*pin[i & 1])
        net.flush()
        torch.cuda.synchronize()
        im2, bx2 = _inputs(dev, 75, 125, 40, seed=1)
        net.set_scales([60, 75])                                      # pyramid maps; the rescaled image and its temporary
        net.test_one_async(im2, bx2)
        net.set_scales([])
        net.set_augment(True)                                         # the mirrored half's buffers
        net.test_one_async(im, bx)
        net.set_augment(False)
        torch.cuda.synchronize()
        before_train = _live(lib)
        net.train_begin(depth=2)
        assert _live(lib)[0] > before_train[0]
        labels = torch.from_numpy((np.arange(16) % 4).astype(np.int32)).to(dev)
        net.train_add(im, bx[:16].contiguous(), bx[:16].contiguous(), labels)
        net.train_step(0.01)
        torch.cuda.synchronize()
        net.train_end()
        assert _live(lib) == before_train                             # at train_end, not at handle destruction
        net.set_graphs(True)                                          # capture stream
        for _ in range(2):
            net.test_one_async(im, bx)
        torch.cuda.synchronize()
        net.set_graphs(False)
        net.set_profiling(True)                                       # the timing events' pool
        net.test_one_async(im, bx)
        torch.cuda.synchronize()
        net.get_profile()
        net.set_profiling(False)
        assert net.debug_tensor("cls", (64, 4)).shape == (64, 4)      # the debug buffer
        held = _live(lib)
        assert held[1] - start[1] >= 3 and held[2] - start[2] >= 4    # side, copy and capture streams; head / tail events
        net.close()
        assert _live(lib) == start


@pytest.mark.parametrize("fc_arith", ["fp32", "split3"])
def test_mpnet_handle_returns_everything(dev, fc_arith):
    with _lib.debug_hooks() as lib:
        start = _live(lib)
        net = _mpnet(128, fc_arith=fc_arith)
        held = _live(lib)
        assert held[0] - start[0] >= 9 and held[1] - start[1] >= 2 and held[2] - start[2] >= 9
        net.test_one_async(*_inputs(dev, 150, 250, 120))
        torch.cuda.synchronize()
        net.close()
        assert _live(lib) == start


@pytest.mark.parametrize("model", ["rn_mpn_bf16", "rn_mpn_f32", "inc_mpn_bf16", "alexnet"])
def test_graph_net_handle_returns_everything(dev, model):
    """ResNet and op-list handles (test_gpu_pipeline.py's test-size towers, test_gpu_launch_graphs.py's AlexNet): the ResNetGraph object
    has an owner of its own; a second, larger image regrows whatever is sized by the image."""
    with _lib.debug_hooks() as lib:
        start = _live(lib)
        if model.startswith("rn"):
            R = models.synthetic_resnet_mpn_params(depth=0, n_classes=7, n_integral=3, base_width=16, blocks=[1, 1, 1, 2], block_type="bottleneck", seed=31)
            H, W, n_conv = 150, 250, 10
            net = models.ResNetFRCNN(R, max_h=H, max_w=W, max_rois=200, top_k=20, bf16=model.endswith("bf16"))
        elif model == "alexnet":
            G = models.synthetic_alexnet_params(n_classes=6, seed=5, width=0.25, fc_dim=256)
            H, W, n_conv = 160, 208, 5
            net = models.AlexNetFRCNN(G, max_h=H, max_w=W, max_rois=64, top_k=10)
        else:
            G = models.synthetic_inception_mpn_params(n_classes=5, n_integral=2, width=0.25, seed=17)
            H, W, n_conv = 170, 215, 10
            net = models.InceptionFRCNN(G, max_h=H, max_w=W, max_rois=120, top_k=10, bf16=True)
        assert _live(lib)[0] - start[0] >= n_conv
        net.test_one_async(*_inputs(dev, H - 30, W - 40, 50))
        net.test_one_async(*_inputs(dev, H, W, 50, seed=1))
        torch.cuda.synchronize()
        net.close()
        assert _live(lib) == start
