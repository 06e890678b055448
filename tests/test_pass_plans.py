"""The plans of the descriptor passes, as literal numbers: what uz_X_workspace_bytes / uz_X_grid (uz_patch_index_bytes /
uz_patch_cut_grid) answer for each of the ten descriptor types at three descriptors.  The host code that forms these plans
is shared (csrc/uz_host.h); the numbers are what every captured graph and every workspace allocation was sized by, so they
are pinned here.  CPU only: the calls launch nothing."""
import pytest

from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops

# (N, C, H, W, class mode): the smallest; an odd one (no multiple of a tile, the class mode where the pass has one); one
# where the eight-workgroups-per-CU cap is reached and workgroups walk (tests/test_boundary_loss.py::test_grid_reports_the_column_pass)
SHAPES = {"small": (2, 1, 8, 8, False), "odd": (2, 3, 33, 20, True), "walk": (9, 1, 256, 256, False)}


def _region(N, C, H, W, cls):
    return L.RegionDesc(1, N * C * H * W, N * C, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 1.0, 0)


def _class(N, C, H, W, cls):
    return L.ClassDesc(1, N, max(C, 2), H * W, 1.0, 1.0, 1.0, 0.0, -100, L.CLASS_REDUCE_BATCH, 0, 0, 0)      # K >= 2 always


def _augment(N, C, H, W, cls):
    return L.AugmentDesc(N, C, H, W, L.AUGMENT_MASK_I32 if cls else L.AUGMENT_MASK_F32, 1, 0, 0.5, 0.5, 0.3, 0.8, 1.2, 0.1, 0.2, 0.2,
                         0.0, 0.0, 0)


def _patch(N, C, H, W, cls):      # a pool of N pictures, N patches of the whole picture
    return L.PatchDesc(N, C, H, W, L.PATCH_IMAGE_F32, L.PATCH_MASK_I32 if cls else L.PATCH_MASK_F32, 1, 2 if cls else 1, N, H, W, 0,
                       0.5, 0.0)


def _surface(N, C, H, W, cls):
    return L.SurfaceDesc(L.SURFACE_CLASS if cls else L.SURFACE_BINARY, N, C, H, W, 1 if cls else 0, -100, 0, 95.0, 1.0)


def _confusion(N, C, H, W, cls):
    return L.ConfusionDesc(L.CONFUSION_CLASS if cls else L.CONFUSION_BINARY, N, C, H, W, 1 if cls else 0, -100, 0 if cls else 64, 0)


def _boundary(N, C, H, W, cls):
    return L.BoundaryDesc(L.BOUNDARY_CLASS if cls else L.BOUNDARY_BINARY, 1, N, C, H, W, 1 if cls else 0, -100, 0, 1.0)


def _lovasz(N, C, H, W, cls):
    return L.LovaszDesc(L.LOVASZ_CLASS if cls else L.LOVASZ_BINARY, 1, N, C, H, W, 1, L.LOVASZ_PRESENT, -100, 0)


def _cldice(N, C, H, W, cls):
    return L.ClDiceDesc(L.CLDICE_CLASS if cls else L.CLDICE_BINARY, 1, N, C, H, W, 0, 0, -100, 3, 1.0, 0)


def _postproc(N, C, H, W, cls):
    return L.PostprocDesc(L.POST_CLASS if cls else L.POST_BINARY, N, C, H, W, 1 if cls else 0, 1, 0, 0, 0, 0.5, 0)


# pass -> (descriptor, bytes query or None, grid query or None)
PASSES = {
    "region": (_region, L.region_loss_workspace_bytes, None),
    "class": (_class, L.class_loss_workspace_bytes, None),
    "augment": (_augment, None, ops.augment_grid),
    "patch": (_patch, ops.patch_index_bytes, ops.patch_cut_grid),
    "surface": (_surface, L.surface_workspace_bytes, L.surface_grid),
    "confusion": (_confusion, L.confusion_workspace_bytes, L.confusion_grid),
    "boundary": (_boundary, L.boundary_workspace_bytes, L.boundary_grid),
    "lovasz": (_lovasz, L.lovasz_workspace_bytes, L.lovasz_grid),
    "cldice": (_cldice, L.cldice_workspace_bytes, L.cldice_grid),
    "postproc": (_postproc, L.postproc_workspace_bytes, L.postproc_grid),
}


def plan(name, shape):
    """(bytes or None, (workgroups, units) or None) of pass `name` at SHAPES[shape]"""
    desc, nbytes, grid = PASSES[name]
    d = desc(*SHAPES[shape])
    return (nbytes(d) if nbytes else None, grid(d) if grid else None)


# Recorded from the library built from the commit BEFORE the host scaffold (54b331f, where every pass carried its own copy
# of the range / align / carve / cap code): plan(name, shape) for every pair, printed by a throw-away script.  A plan that
# moves changes workspace sizes or launch grids, which this refactor must not.
WANT = {
    ("region", "small"): (128, None),
    ("region", "odd"): (384, None),
    ("region", "walk"): (7056, None),
    ("class", "small"): (496, None),
    ("class", "odd"): (672, None),
    ("class", "walk"): (57680, None),
    ("augment", "small"): (None, (2, 2)),
    ("augment", "odd"): (None, (2, 2)),
    ("augment", "walk"): (None, (576, 576)),
    ("patch", "small"): (72, (2, 2)),
    ("patch", "odd"): (544, (2, 2)),
    ("patch", "walk"): (9252, (576, 576)),
    ("surface", "small"): (133008, (4, 4)),
    ("surface", "odd"): (296944, (24, 24)),
    ("surface", "walk"): (8903088, (2048, 4608)),
    ("confusion", "small"): (1056, (2, 2)),
    ("confusion", "odd"): (80, (2, 2)),
    ("confusion", "walk"): (4752, (576, 576)),
    ("boundary", "small"): (464, (2, 2)),
    ("boundary", "odd"): (6512, (12, 12)),
    ("boundary", "walk"): (1214752, (2048, 2304)),
    ("lovasz", "small"): (6224, (2, 2)),
    ("lovasz", "odd"): (75840, (6, 6)),
    ("lovasz", "walk"): (10045568, (576, 576)),
    ("cldice", "small"): (1136, (2, 2)),
    ("cldice", "odd"): (47840, (8, 8)),
    ("cldice", "walk"): (4737072, (576, 576)),
    ("postproc", "small"): (2336, (2, 2)),
    ("postproc", "odd"): (27232, (12, 12)),
    ("postproc", "walk"): (5921280, (2048, 2304)),
}


@pytest.mark.parametrize("name", sorted(PASSES))
def test_plans_are_the_recorded_ones(name):
    for shape in SHAPES:
        assert plan(name, shape) == WANT[name, shape], (name, shape)


def test_the_table_covers_every_pass_and_the_walk_case_walks():
    assert set(WANT) == {(n, s) for n in PASSES for s in SHAPES} and len(PASSES) == 10
    for name in ("surface", "boundary", "postproc"):      # 256-pixel units: more of them than the 2048 workgroups, the rest is walked
        grid, units = WANT[name, "walk"][1]
        assert grid == 2048 and units > grid, name
    for name in PASSES:      # every workspace ends on a 16-byte boundary (the patch index is no workspace: 4-byte counts)
        for shape in SHAPES:
            nbytes = WANT[name, shape][0]
            assert nbytes is None or nbytes % (4 if name == "patch" else 16) == 0
