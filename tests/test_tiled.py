"""CPU: the tile plan of SlidingWindowPredict, the refusals of the uz_tile_* entries (the library loads without a GPU) and the
argument checks of the class.  tests/tile_ref.py restates the plan; uz_tile_plan is what Python and the kernels both use."""
import ctypes

import numpy as np
import pytest
import torch

import tile_ref as T  # tests/tile_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.postprocess import MaskPostprocess
from unet_zoo_amd.tiled import SlidingWindowPredict

WINDOWS, OVERLAPS = (7, 32, 64), (0.0, 0.25, 0.5, 0.75)


# ---- uz_tile_plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_plan_is_the_reference_plan_and_covers_every_pixel(window):
    most = 0
    for overlap in OVERLAPS:
        for size in range(1, 201):
            want = T.plan(size, window, overlap)
            got = ops.tile_plan(size, window, overlap)               # (at most 194 tiles, window 7 at overlap 0.75)
            assert got == want, (size, window, overlap)
            D = max(size, window)
            assert got[0] == 0 and all(0 <= s <= D - window for s in got)          # no tile leaves the canvas
            assert all(b > a for a, b in zip(got, got[1:]))
            k = T.cover(got, window, size)
            assert k.min() >= 1 and k.max() <= _lib.TILE_MAX_COVER, (size, window, overlap, k.max())
            most = max(most, int(k.max()))
    # overlap 0.75: window / step tiles, and the shifted last tile among them adds one (window 7: step 1, every start is taken)
    assert most == {7: 7, 32: 5, 64: 5}[window]


def test_plan_by_hand_and_its_refusals():
    assert ops.tile_plan(72, 32, 0.5) == [0, 16, 32, 40] and ops.tile_plan(88, 32, 0.5) == [0, 16, 32, 48, 56]
    assert ops.tile_plan(24, 32, 0.5) == [0] and ops.tile_plan(32, 32, 0.75) == [0] and ops.tile_plan(64, 32, 0.0) == [0, 32]
    assert ops.tile_plan(33, 32, 0.0) == [0, 1] and ops.tile_plan(1024, 256, 0.5) == [0, 128, 256, 384, 512, 640, 768]
    lib = _lib.load()
    buf = (ctypes.c_int * 256)()
    for args, word in (((0, 32, 0.5, buf, 64), b"positive"), ((32, 0, 0.5, buf, 64), b"positive"), ((64, 32, -0.1, buf, 64), b"overlap"),
                       ((64, 32, 0.76, buf, 64), b"overlap"), ((64, 32, float("nan"), buf, 64), b"overlap"), ((64, 32, 0.5, None, 64), b"null pointer"),
                       ((64, 32, 0.5, buf, 2), b"tiles along an axis"), ((8192, 32, 0.5, buf, 256), b"tiles along an axis")):
        assert lib.uz_tile_plan(*args) == -1 and word in lib.uz_last_error_string(), args
    assert lib.uz_tile_plan(64, 32, 0.5, buf, 3) == 3 and list(buf[:3]) == [0, 16, 32]


# ---- uz_tile_gather / uz_tile_blend without a GPU ------------------------------------------------------------------------------------
def _tab(v):
    return (ctypes.c_int * len(v))(*v)


def _gdesc(N=2, C=3, H=72, W=88, th=32, tw=32, ny=4, nx=5, pad=0, t0=0, tn=40):
    return _lib.TileGatherDesc(N, C, H, W, th, tw, ny, nx, pad, t0, tn, 0)


def _bdesc(N=2, C=3, H=72, W=88, th=32, tw=32, ny=4, nx=5):
    return _lib.TileBlendDesc(N, C, H, W, th, tw, ny, nx)


YS, XS = [0, 16, 32, 40], [0, 16, 32, 48, 56]
X, OUT, TILES, GH, GW = 0x100000, 0x4000000, 0x8000000, 0x200000, 0x300000


def _gather(d, ys=YS, xs=XS, x=X, out=OUT):
    lib = _lib.load()
    rc = lib.uz_tile_gather(ctypes.byref(d) if d is not None else None, _tab(ys) if ys is not None else None, _tab(xs) if xs is not None else None,
                            x, out, None)
    return rc, lib.uz_last_error_string()


def _blend(d, ys=YS, xs=XS, tiles=TILES, gh=GH, gw=GW, out=OUT):
    lib = _lib.load()
    rc = lib.uz_tile_blend(ctypes.byref(d) if d is not None else None, _tab(ys) if ys is not None else None, _tab(xs) if xs is not None else None,
                           tiles, gh, gw, out, None)
    return rc, lib.uz_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(N=0), b"shape"), (dict(C=0), b"shape"), (dict(H=-1), b"shape"), (dict(W=0), b"shape"), (dict(th=0), b"window"), (dict(tw=-2), b"window"),
    (dict(ny=0), b"tiles along H"), (dict(nx=257), b"tiles along W"), (dict(N=1 << 20, C=64), b"too large"), (dict(H=80), b"do not run from 0"),
    (dict(W=100), b"do not run from 0")])
def test_both_entries_refuse_a_bad_descriptor_without_a_gpu(kw, word):
    for call, make in ((_gather, _gdesc), (_blend, _bdesc)):
        rc, msg = call(make(**kw))
        assert rc == -1 and word in msg, (call.__name__, msg)


def test_entry_specific_refusals_without_a_gpu():
    for kw, word in ((dict(pad=2), b"pad_mode"), (dict(t0=-1), b"outside the list"), (dict(tn=0), b"outside the list"), (dict(t0=39, tn=2), b"outside the list")):
        rc, msg = _gather(_gdesc(**kw))
        assert rc == -1 and word in msg, msg
    # reflect: a 24-row image in a 32-row window is padded by 4 < 24; an 8-row image by 12 >= 8
    rc, msg = _gather(_gdesc(N=1, H=8, W=50, ny=1, nx=2, pad=1, tn=2), ys=[0], xs=[0, 18])
    assert rc == -1 and b"reflect needs pad < size" in msg
    rc, msg = _gather(_gdesc(N=1, H=8, W=50, ny=1, nx=2, pad=0, tn=2), ys=[0], xs=[0, 18], x=None)      # ... zero padding passes that check
    assert rc == -1 and b"null pointer" in msg
    # N ny nx C th tw >= 2^31 although N C H W = 2^29: 125 x 125 windows of 256 at overlap 0.75 on 8192 x 8192
    big = list(range(0, 7937, 64))
    rc, msg = _blend(_bdesc(N=1, C=8, H=8192, W=8192, th=256, tw=256, ny=125, nx=125), ys=big, xs=big)
    assert rc == -1 and b"T C th tw" in msg


def test_start_tables_are_checked_without_a_gpu():
    for call, make in ((_gather, _gdesc), (_blend, _bdesc)):
        for ys, word in (([0, 16, 16, 40], b"not ascending"), ([0, 3, 36, 40], b"leave a gap"), ([1, 16, 32, 40], b"do not run from 0"),
                         ([0, 16, 32, 39], b"do not run from 0")):
            rc, msg = call(make(), ys=ys)
            assert rc == -1 and word in msg, (ys, msg)
        rc, msg = call(make(W=40, nx=9), xs=list(range(9)))                   # nine tiles over the pixel 8
        assert rc == -1 and b"9 tiles cover one pixel along W" in msg
        assert call(None)[0] == -1 and b"null descriptor" in call(None)[1]
        for k in ("ys", "xs"):
            rc, msg = call(make(), **{k: None})
            assert rc == -1 and b"null pointer" in msg


def test_null_pointers_misalignment_and_overlaps_are_refused_without_a_gpu():
    for kw in (dict(x=None), dict(out=None)):
        rc, msg = _gather(_gdesc(), **kw)
        assert rc == -1 and b"null pointer" in msg
    for kw in (dict(tiles=None), dict(gh=None), dict(gw=None), dict(out=None)):
        rc, msg = _blend(_bdesc(), **kw)
        assert rc == -1 and b"null pointer" in msg
    for kw in (dict(x=X + 2), dict(out=OUT + 1)):
        rc, msg = _gather(_gdesc(), **kw)
        assert rc == -1 and b"4-byte" in msg
    for kw in (dict(tiles=TILES + 2), dict(gh=GH + 1), dict(gw=GW + 2), dict(out=OUT + 2)):
        rc, msg = _blend(_bdesc(), **kw)
        assert rc == -1 and b"4-byte" in msg
    nx_bytes, tile_bytes = 4 * 2 * 3 * 72 * 88, 4 * 40 * 3 * 32 * 32
    for out in (X, X + nx_bytes - 4, X - tile_bytes + 4):
        rc, msg = _gather(_gdesc(), out=out)
        assert rc == -1 and b"overlaps" in msg, hex(out)
    for kw in (dict(out=TILES), dict(out=TILES + tile_bytes - 4), dict(out=GH + 4 * 31), dict(out=GW - nx_bytes + 4)):
        rc, msg = _blend(_bdesc(), **kw)
        assert rc == -1 and b"overlaps" in msg, kw


# ---- ops and the class (no GPU) ----------------------------------------------------------------------------------------------------
def test_tile_weights():
    assert torch.equal(ops.tile_weights(5, "constant"), torch.ones(5))
    g = ops.tile_weights(32, "gaussian", 0.125)
    i = np.arange(32, dtype=np.float64)
    want = np.exp(-(i - 15.5) ** 2 / (2 * (0.125 * 32) ** 2)).astype(np.float32)
    assert g.dtype == torch.float32 and np.array_equal(g.numpy(), want) and torch.equal(g, g.flip(0))
    with pytest.raises(ValueError, match="unknown window weight"):
        ops.tile_weights(8, "hann")
    with pytest.raises(ValueError, match="sigma_scale"):
        ops.tile_weights(8, "gaussian", 0.0)


def test_ops_refuse_cpu_tensors_and_unknown_padding():
    x, out = torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8)
    with pytest.raises(_lib.HipLibraryError):
        ops.tile_gather(x, [0], [0], (8, 8), "constant", 0, out)
    with pytest.raises(_lib.HipLibraryError):
        ops.tile_blend(x, [0], [0], torch.ones(8), torch.ones(8), out)


@pytest.fixture(scope="module")
def model():
    return unet_zoo_amd.create_model("unet").eval()


@pytest.mark.parametrize("kw,err,word", [
    (dict(window=32), ValueError, "two positive ints"), (dict(window=(32,)), ValueError, "two positive ints"),
    (dict(window=(32, 0)), ValueError, "two positive ints"), (dict(window=(32.0, 32)), ValueError, "two positive ints"),
    (dict(window=(32, True)), ValueError, "two positive ints"), (dict(window="ab"), ValueError, "two positive ints"),
    (dict(overlap=-0.1), ValueError, "overlap"), (dict(overlap=0.8), ValueError, "overlap"), (dict(overlap="half"), ValueError, "overlap"),
    (dict(blend="hann"), ValueError, "unknown blend"), (dict(sigma_scale=0), ValueError, "sigma_scale"),
    (dict(pad_mode="replicate"), ValueError, "unknown pad_mode"), (dict(tta=("rot90",)), ValueError, "unknown view"),
    (dict(tta="hflip"), ValueError, "sequence"), (dict(tile_batch=0), ValueError, "tile_batch"), (dict(tile_batch=2.0), ValueError, "tile_batch"),
    (dict(postprocess=object()), TypeError, "MaskPostprocess"), (dict(mode="multi"), ValueError, "mode must be")])
def test_constructor_refuses_bad_arguments_by_name(model, kw, err, word):
    args = dict(window=(32, 32))
    args.update(kw)
    with pytest.raises(err, match=word):
        SlidingWindowPredict(model, **args)


def test_constructor_refuses_a_training_model_and_a_foreign_module():
    with pytest.raises(RuntimeError, match="eval"):
        SlidingWindowPredict(unet_zoo_amd.create_model("unet"), window=(32, 32))       # a fresh model is in train mode
    with pytest.raises(TypeError, match="HipModule"):
        SlidingWindowPredict(torch.nn.Conv2d(1, 1, 1), window=(32, 32))


def test_shape_dependent_refusals_come_before_any_gpu_call(model):
    pred = SlidingWindowPredict(model, window=(32, 32), pad_mode="reflect", tile_batch=16, tta=("hflip",), postprocess=MaskPostprocess())
    plan = pred.plan_for((2, 3, 72, 88))
    assert plan["ys"] == [0, 16, 32, 40] and plan["xs"] == [0, 16, 32, 48, 56] and plan["tiles_per_image"] == 20 and plan["tiles"] == 40
    assert plan["batches"] == [(0, 16), (16, 16), (32, 8)] and plan["forwards"] == 6
    assert pred.plan_for((1, 3, 24, 50))["xs"] == [0, 16, 18]                            # padded by 4 rows each side: fine
    with pytest.raises(ValueError, match="reflect padding needs pad < size"):
        pred.plan_for((1, 3, 8, 50))                                                    # 12 rows below an 8-row image
    with pytest.raises(ValueError, match="reflect padding needs pad < size"):
        pred(torch.zeros(1, 3, 8, 50))                                                  # (the same error before the device is looked at)
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        pred.plan_for((3, 72, 88))
    big = SlidingWindowPredict(model, window=(256, 256), overlap=0.75)
    with pytest.raises(ValueError, match="2\\^31 elements"):
        big.plan_for((32, 3, 2048, 2048), channels=2)                                   # 32 x 841 tiles x 2 x 256 x 256
    assert big.plan_for((32, 3, 2048, 2048), channels=1)["tiles"] == 32 * 841
    with pytest.raises(ValueError, match="2\\^31 elements"):
        big(torch.zeros(1).expand(64, 3, 2048, 2048))                                   # ... already with one channel
    with pytest.raises(_lib.HipLibraryError, match="tiles along an axis"):
        SlidingWindowPredict(model, window=(7, 7), overlap=0.75).plan_for((1, 3, 1000, 1000))
    with pytest.raises(RuntimeError, match="no CPU path"):                              # good arguments on the CPU: no fallback
        pred(torch.zeros(1, 3, 72, 88))
    assert "gather+flip+2 x fwd+merge" in pred.describe() and "reflect" in pred.describe()


def test_exports_and_descriptor_sizes():
    assert unet_zoo_amd.SlidingWindowPredict is SlidingWindowPredict and "SlidingWindowPredict" in unet_zoo_amd.__all__
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uz_tile_plan", "uz_tile_gather", "uz_tile_blend"):
        assert name in _lib.EXPORTS and getattr(raw, name)
    assert ctypes.sizeof(_lib.TileGatherDesc) == 48 and ctypes.sizeof(_lib.TileBlendDesc) == 32
    assert (_lib.TILE_MAX_AXIS, _lib.TILE_MAX_COVER) == (256, 8) and T.MAX_COVER == _lib.TILE_MAX_COVER
    assert _lib.TILE_PADS == {"constant": 0, "reflect": 1}
