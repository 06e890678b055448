"""CPU: the reference of LovaszLoss (tests/lovasz_ref.py) against Berman's published form (sort, cumsum, Jaccard, differences),
the closed-form weights, the defining property (errors in {0, 1}: the Jaccard loss of the mispredicted set, brute force) and
hand-derived segments; torch's own float32 evaluation of the GPU tests' cases against their bounds; the Python class as far
as it goes without a GPU."""
import itertools

import pytest
import torch

import lovasz_ref as R  # tests/lovasz_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import BoundaryLoss, LovaszLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L


# ---------------------------------------------------------------------------------------------------------- Berman's form
def berman_grad(gt_sorted):
    """the published gradient of the Lovasz extension w.r.t. sorted errors: Jaccard of the prefixes, then differences"""
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if len(gt_sorted) > 1:
        jaccard[1:] = jaccard[1:] - jaccard[:-1]
    return jaccard


def berman_hinge_flat(logits, labels):
    signs = 2.0 * labels - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
    return torch.dot(torch.relu(errors_sorted), berman_grad(labels[perm]))


def berman_softmax_flat(probas, labels, present_only):
    """probas (P, K), labels (P): the mean over the (present) classes"""
    losses = []
    for c in range(probas.shape[1]):
        fg = (labels == c).double()
        if present_only and fg.sum() == 0:
            continue
        errors_sorted, perm = torch.sort((fg - probas[:, c]).abs(), 0, descending=True)
        losses.append(torch.dot(errors_sorted, berman_grad(fg[perm])))
    return sum(losses) / len(losses) if losses else torch.zeros((), dtype=torch.float64)


@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_binary_term_equals_bermans_hinge(seed, per_image):
    g = torch.Generator().manual_seed(seed)
    x = (2.0 * torch.randn(3, 2, 7, 5, generator=g)).double()
    t = (torch.rand(3, 2, 7, 5, generator=g) > 0.6).double()
    t[1, 0] = 0.0                      # an empty plane: max(e, 0)
    t[2, 1] = 1.0
    V, _, _ = R.term(x, t, False, per_image)
    if per_image:
        want = sum(berman_hinge_flat(x[n, c].reshape(-1), t[n, c].reshape(-1)) for n in range(3) for c in range(2)) / 6
    else:
        want = sum(berman_hinge_flat(x[:, c].reshape(-1), t[:, c].reshape(-1)) for c in range(2)) / 2
    # the reference takes e in fp32 (one rounding of a value below 16): 2^-21 absolute per element, weights sum to <= 1
    assert abs(V.item() - want.item()) < 1e-6


@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("per_image", [True, False])
def test_class_term_equals_bermans_softmax(per_image, classes):
    g = torch.Generator().manual_seed(3)
    N, K, H, W = 3, 5, 6, 7
    x = torch.randn(N, K, H, W, generator=g).double()
    y = torch.randint(0, K, (N, H, W), generator=g)
    y[0][y[0] == 2] = 1                # image 0 lacks class 2
    y[:, 2, :] = -100
    y[1, 0, 0] = K + 1
    V, _, _ = R.term(x, y, True, per_image, classes)
    p = torch.softmax(x, 1).permute(0, 2, 3, 1)
    valid = (y >= 0) & (y < K)
    if per_image:
        want = sum(berman_softmax_flat(p[n][valid[n]], y[n][valid[n]], classes == "present") for n in range(N)) / N
    else:
        want = berman_softmax_flat(p[valid], y[valid], classes == "present")
    assert abs(V.item() - want.item()) < 1e-12


def test_an_image_without_a_valid_pixel_adds_nothing_and_still_counts():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 4, 4, generator=g).double()
    y = torch.randint(0, 3, (2, 4, 4), generator=g)
    y[1] = -100
    V, e, ranks = R.term(x, y, True, True, "present")
    V0, _, _ = R.term(x[:1], y[:1], True, True, "present")
    assert abs(V.item() - V0.item() / 2) < 1e-15 and (ranks[3:] == -1).all() and not e[3:].any()


# ------------------------------------------------------------------------------------------------------- the weights themselves
def test_closed_form_weights_equal_the_jaccard_differences():
    g = torch.Generator().manual_seed(5)
    b = torch.rand(40, 37, generator=g) > torch.rand(40, 1, generator=g)
    b[0] = False                       # G = 0
    b[1] = True                        # G = the length
    G = b.double().sum(1, keepdim=True)
    a, c = R.weights_sorted(b, G), R.weights_closed_form(b, G)
    assert (a - c).abs().max() < 1e-15
    assert torch.equal(c[0], torch.eye(37, dtype=torch.float64)[0]) and (c[1] - 1.0 / 37).abs().max() < 1e-17
    assert (c >= 0).all() and (c.sum(1) - 1.0).abs().max() < 1e-14          # the differences of J telescope to J_last = 1


def test_errors_in_0_1_give_the_jaccard_loss_of_the_mispredicted_set():
    """the defining property of the Lovasz extension, brute force over every labelling and every error set of 6 pixels"""
    for bits, errs in itertools.product(itertools.product([0, 1], repeat=6), repeat=2):
        b = torch.tensor([bits], dtype=torch.bool)
        e = torch.tensor([errs], dtype=torch.float64)
        values, _, _ = R.segment_values(e, b)
        fg = set(i for i in range(6) if bits[i])
        pred = set(i for i in range(6) if bits[i] != errs[i])          # the prediction: the labelling with the errors flipped
        union = len(fg | pred)
        want = 1.0 - len(fg & pred) / union if union else 0.0
        assert abs(values.item() - want) < 1e-14, (bits, errs)


def _seg(e, b, ranks=None):
    values, ranks, g = R.segment_values(torch.tensor([e], dtype=torch.float64), torch.tensor([b], dtype=torch.bool), ranks)
    return values.item(), ranks[0].tolist(), g[0]


def test_hand_derived_segments():
    # G = 2: ranks by descending e; J = 1 - (G - c) / (G + n) along the ranks
    # e:      0.9(b=0)  0.8(b=1)  0.5(b=0)  0.2(b=1)   ->  J = 1 - 2/3, 1 - 1/3, 1 - 1/4, 1   ->  g = 1/3, 1/3, 1/12, 1/4
    v, r, g = _seg([0.8, 0.9, 0.2, 0.5], [1, 0, 1, 0])
    assert r == [1, 0, 3, 2]
    assert torch.allclose(g, torch.tensor([1 / 3, 1 / 3, 1 / 4, 1 / 12], dtype=torch.float64), atol=1e-15)
    assert abs(v - (0.9 / 3 + 0.8 / 3 + 0.5 / 12 + 0.2 / 4)) < 1e-15
    # G = 0: the largest error alone, the empty target's max(e, 0)
    v, r, g = _seg([0.3, 0.7, -0.1, 0.7, 0.2], [0, 0, 0, 0, 0])
    assert r == [2, 0, -1, 1, 3] and g.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and v == 0.7
    v, r, g = _seg([-1.0, 0.0, -0.5, -2.0], [0, 0, 0, 0])
    assert r == [-1, -1, -1, -1] and v == 0.0 and not g.any()          # no ranked element: L = 0
    # G = the length: every weight 1 / G
    v, r, g = _seg([0.5, 0.25, 1.0, 0.75], [1, 1, 1, 1])
    assert r == [2, 3, 0, 1] and torch.allclose(g, torch.full((4,), 0.25, dtype=torch.float64)) and abs(v - 0.625) < 1e-15
    # ties keep their positions' order, and an unranked member still counts in G (= 3 here)
    #   ranked: pos 0 (e 0.5, b 1), pos 2 (0.5, b 0), pos 3 (0.5, b 1), pos 5 (0.1, b 0); pos 1 (b 1) and pos 4 are unranked
    #   c = 1, 1, 2, 2; n = 0, 1, 1, 2; J = 1 - 2/3, 1 - 2/4, 1 - 1/4, 1 - 1/5 -> g = 1/3, 1/6, 1/4, 1/20
    v, r, g = _seg([0.5, 0.0, 0.5, 0.5, -0.3, 0.1], [1, 1, 0, 1, 0, 0])
    assert r == [0, -1, 1, 2, -1, 3]
    assert torch.allclose(g, torch.tensor([1 / 3, 0, 1 / 6, 1 / 4, 0, 1 / 20], dtype=torch.float64), atol=1e-15)
    assert abs(v - (0.5 * (1 / 3 + 1 / 6 + 1 / 4) + 0.1 / 20)) < 1e-15
    # another order of the tied elements changes the weights but not the value
    v2, _, g2 = _seg([0.5, 0.0, 0.5, 0.5, -0.3, 0.1], [1, 1, 0, 1, 0, 0], torch.tensor([[2, -1, 0, 1, -1, 3]]))
    assert abs(v2 - v) < 1e-15 and not torch.allclose(g2, g)


def test_binary_gradient_is_minus_s_g_over_the_segments():
    x, t = R.make_inputs((3, 1, 17, 23))
    leaf = x.double().requires_grad_(True)
    V, _, _ = R.term(leaf, t, False, True)
    (grad,) = torch.autograd.grad(V, leaf)
    e, b = R.binary_segments(x, t, True)
    _, ranks, g = R.segment_values(e, b)
    want = torch.where(b, -g, g) / 3
    assert (grad.reshape(3, -1) - want).abs().max() < 1e-16 and not grad.reshape(3, -1)[ranks < 0].any()
    assert (ranks[1] >= 0).sum() > 1 and (g[1] > 0).sum() == 1             # the empty image: one pixel carries the gradient


# ----------------------------------------------------------------------- float32 against float64 on the cases of the GPU tests
def test_float32_evaluation_of_the_gpu_cases_stays_inside_their_bounds():
    """|V32 - V64| against 2e-6 max(1, |V64|) and max |dV32 - dV64| against 2e-6 max |dV64| for torch's own float32
    evaluation (autograd) of every case of tests/test_lovasz_loss_gpu.py; the largest shares are printed (and written into
    that file's docstring).

    ONE kind of case cannot hold the gradient bound in plain float32: the class mode with per_image=True and classes="all",
    where an image lacks a class.  That segment has G = 0, so its top-ranked pixel alone carries 1 / (N K) -- hundreds of
    times any other weight -- and it is the pixel where the absent class is most probable: p = 0.993 at K = 4, and
    p_k (d_k - sum_c p_c d_c) then subtracts two numbers that agree in their first two digits.  torch's float32 autograd lands at
    2.2 (K = 4) and 3.0 (K = 8) times the bound there.  The bound is not widened for it: the kernel takes the difference for the
    class of the largest logit as d (1 - p) - sum_{c != top} p_c d_c with 1 - p = sum_{c != top} p_c (no difference of
    near-equals; lovasz_ref.class_grad_float32_top restates that form in float32), which stays below 0.2 of the bound on
    every class case."""
    worst_v, worst_g, worst_top = 0.0, 0.0, 0.0
    cases = [(R.make_inputs(s), False, pi, "present") for s in R.SHAPES for pi in (True, False)]
    cases += [(R.make_tied_inputs((2, 1, 40, 40)), False, pi, "present") for pi in (True, False)]
    cases += [(R.make_class_inputs(K), True, pi, cl) for K in (4, 8) for pi in (True, False) for cl in ("present", "all")]
    for (x, t), cls, per_image, classes in cases:
        leaf = x.double().requires_grad_(True)
        V64, _, _ = R.term(leaf, t, cls, per_image, classes)
        (g64,) = torch.autograd.grad(V64, leaf)
        V32, g32 = R.term_float32(x, t, cls, per_image, classes)
        bound = 2e-6 * g64.abs().max().item()
        sv = abs(V32.item() - V64.item()) / (2e-6 * max(1.0, abs(V64.item())))
        sg = (g32.double() - g64).abs().max().item() / bound
        print(f"{tuple(x.shape)} class={cls} per_image={per_image} {classes}: value {sv:.3f} gradient {sg:.3f}")
        assert sv < 1.0
        worst_v = max(worst_v, sv)
        if cls:
            top = (R.class_grad_float32_top(x, t, per_image, classes).double() - g64).abs().max().item() / bound
            print(f"    the kernel's form of the gradient in float32: {top:.3f}")
            worst_top = max(worst_top, top)
        if cls and per_image and classes == "all":
            assert 1.0 < sg < 10.0, sg              # the reported case: plain float32 cannot hold the bound, the kernel's form does
        else:
            assert sg < 1.0, (tuple(x.shape), cls, per_image, classes, sg)
            worst_g = max(worst_g, sg)
    print(f"largest share of the bound: value {worst_v:.3f}, gradient {worst_g:.3f}, the kernel's class-mode form {worst_top:.3f}")
    assert worst_v < 0.5 and worst_g < 0.5 and worst_top < 0.5


# ---------------------------------------------------------------------------------------------------------- the Python class
def test_package_exports_it():
    assert "LovaszLoss" in unet_zoo_amd.__all__ and unet_zoo_amd.LovaszLoss is LovaszLoss


def test_constructor_refusals_and_accepted_edges():
    for bad in ("dice", 3, None, lambda o, t: 0, BoundaryLoss(), LovaszLoss()):      # stacking is out of scope
        with pytest.raises(TypeError, match="LovaszLoss: base"):
            LovaszLoss(base=bad)
    with pytest.raises(TypeError, match="BoundaryLoss: base"):
        BoundaryLoss(base=LovaszLoss())
    for kw in (dict(weight=-1e-3), dict(base_scale=-1.0), dict(weight=float("nan")), dict(base_scale=float("inf")),
               dict(weight=0.0, base_scale=0.0), dict(weight="much"), dict(classes="some"), dict(classes=None)):
        with pytest.raises(ValueError, match="LovaszLoss:"):
            LovaszLoss(**kw)
    c = LovaszLoss()
    assert c.base == "bce_dice" and c.weight == 1.0 and c.base_scale == 1.0 and c.per_image and c.classes == "present"
    assert LovaszLoss(weight=0.0).weight == 0.0 and LovaszLoss(base_scale=0.0).base_scale == 0.0
    assert not LovaszLoss(base=RegionLoss.dice(), per_image=False, classes="all").per_image
    assert "LovaszLoss(" in repr(c) and c.errors is None and c.ranks is None and c.term is None


def test_set_weights_validates():
    c = LovaszLoss(base=RegionLoss.dice())
    c.set_weights(weight=0.5)
    assert (c.weight, c.base_scale) == (0.5, 1.0)
    c.set_weights(base_scale=0.0)
    assert (c.weight, c.base_scale) == (0.5, 0.0)
    for kw in (dict(weight=-1.0), dict(base_scale=float("nan")), dict(weight=0.0), dict(weight=float("inf"))):
        with pytest.raises(ValueError, match="LovaszLoss:"):
            c.set_weights(**kw)
    assert (c.weight, c.base_scale) == (0.5, 0.0)              # a refused call changes nothing


def test_target_dtype_ignore_index_and_weights_follow_the_base():
    assert LovaszLoss().target_dtype == torch.float32 and not LovaszLoss(base=RegionLoss()).class_mode
    c = LovaszLoss(base=MulticlassLoss(ignore_index=255))
    assert c.target_dtype == torch.int32 and c.class_mode and c.ignore_index == 255
    maps = {"a": torch.zeros(1), "b": torch.zeros(1)}
    assert LovaszLoss().weights_for(maps) == (1.0, 1.0)
    assert LovaszLoss(base=RegionLoss(output_weights={"a": 1, "b": .5})).weights_for(maps) == (1.0, 0.5)


def test_cpu_tensors_and_bad_shapes_are_refused_at_call():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for c in (LovaszLoss(), LovaszLoss(base=RegionLoss())):
        with pytest.raises(L.HipLibraryError):
            c(x, t)
        with pytest.raises(L.HipLibraryError):
            c.direct(x, t)
    with pytest.raises(ValueError, match="LovaszLoss: .*shape"):
        LovaszLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5))
    with pytest.raises(ValueError, match="LovaszLoss: .*integer"):
        LovaszLoss(base=MulticlassLoss())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4))


def test_the_library_refuses_what_it_cannot_sort():
    ok = L.LovaszDesc(L.LOVASZ_BINARY, 1, 16, 1, 512, 512, 0, L.LOVASZ_PRESENT, -100, 0)      # 2^22 in ONE segment
    assert L.lovasz_workspace_bytes(ok) > 16 * (1 << 22) and L.lovasz_grid(ok) == (2048, 4096)
    for bad in (L.LovaszDesc(L.LOVASZ_BINARY, 1, 17, 1, 512, 512, 0, L.LOVASZ_PRESENT, -100, 0),         # a longer segment
                L.LovaszDesc(L.LOVASZ_BINARY, L.CLASS_MAX_ITEMS + 1, 1, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0),
                L.LovaszDesc(L.LOVASZ_CLASS, 1, 1, L.CLASS_MAX_K + 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0),
                L.LovaszDesc(L.LOVASZ_CLASS, 1, 1, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0),
                L.LovaszDesc(L.LOVASZ_BINARY, 16, 65, 1, 512, 512, 1, L.LOVASZ_PRESENT, -100, 0),        # above 2^28 elements
                L.LovaszDesc(2, 1, 1, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0),
                L.LovaszDesc(L.LOVASZ_CLASS, 1, 1, 4, 8, 8, 1, 2, -100, 0),
                L.LovaszDesc(L.LOVASZ_BINARY, 2, 1, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 2),
                L.LovaszDesc(L.LOVASZ_BINARY, 1, 0, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0)):
        assert L.load().uz_lovasz_workspace_bytes(bad) < 0
        with pytest.raises(L.HipLibraryError, match="uz_lovasz_grid"):
            L.lovasz_grid(bad)
    # every shape of the README's table, per image and as one batch segment
    for n, hw in ((16, 256), (16, 512), (8, 512), (1, 1024)):
        for per_image in (1, 0):
            assert L.lovasz_workspace_bytes(L.LovaszDesc(L.LOVASZ_BINARY, 1, n, 1, hw, hw, per_image, 0, -100, 0)) > 0
    assert L.lovasz_workspace_bytes(L.LovaszDesc(L.LOVASZ_BINARY, 7, 8, 1, 512, 512, 1, 0, -100, 0)) > 0      # u2net's seven


def test_null_and_overlapping_pointers_are_refused_before_any_launch():
    import ctypes
    lib = L.load()
    assert lib.uz_lovasz_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_lovasz_grid(None, None) < 0 and b"null descriptor" in lib.uz_last_error_string()
    d = L.LovaszDesc(L.LOVASZ_BINARY, 1, 2, 1, 8, 8, 1, L.LOVASZ_PRESENT, -100, 0)      # 2 x 1 x 8 x 8: maps of 512 bytes
    assert 16 <= L.lovasz_workspace_bytes(d) < 0x10000
    items = (L.LovaszItem * 1)()
    items[0].logits, items[0].dlogits, items[0].weight = 0x10000, 0x20000, 1.0
    # the other pointers at disjoint made-up addresses: nothing is dereferenced before the checks
    ok = dict(target=0x30000, scales=0x40000, base_loss=0x40100, out=0x40200, errors=0x50000, ranks=0x58000, ws=0x100000)

    def call(its=items, **kw):
        a = dict(ok)
        a.update(kw)
        return lib.uz_lovasz_loss(ctypes.byref(d), its, a["target"], a["scales"], a["base_loss"], a["out"], a["errors"], a["ranks"],
                                  a["ws"], None)

    def item(logits, dlogits, weight):
        its = (L.LovaszItem * 1)()
        its[0].logits, its[0].dlogits, its[0].weight = logits, dlogits, weight
        return its

    for name in ok:
        assert call(**{name: None}) < 0 and b"uz_lovasz_loss: null pointer" in lib.uz_last_error_string(), name
    assert lib.uz_lovasz_loss(ctypes.byref(d), None, *ok.values(), None) < 0 and b"null pointer" in lib.uz_last_error_string()
    assert call(its=item(None, 0x20000, 1.0)) < 0 and b"uz_lovasz_loss: item 0 has null logits" in lib.uz_last_error_string()
    assert call(its=item(0x10000, None, -1.0)) < 0 and b"uz_lovasz_loss: item 0 has a negative weight" in lib.uz_last_error_string()
    assert call(ws=0x100008) < 0 and b"uz_lovasz_loss: the workspace must be 16-byte aligned" in lib.uz_last_error_string()
    for kw in (dict(errors=0x50002), dict(ranks=0x58002), dict(out=0x40202), dict(its=item(0x10000, 0x20002, 1.0)),
               dict(its=item(0x10002, 0x20000, 1.0))):
        assert call(**kw) < 0 and b"uz_lovasz_loss: tensors must be 4-byte aligned" in lib.uz_last_error_string(), kw
    for kw in (dict(out=0x40000 + 4), dict(out=0x40100), dict(errors=0x30000 + 256), dict(ranks=0x10000), dict(ws=0x30000 - 16),
               dict(its=item(0x10000, 0x30000 + 128, 1.0)),                                  # every output over an input
               dict(out=0x50000), dict(errors=0x58000 + 4), dict(ranks=0x100000 + 16), dict(ws=0x20000 - 16),
               dict(its=item(0x10000, 0x50000 + 64, 1.0)), dict(its=item(0x10000, 0x58000 - 64, 1.0)),      # every output over another
               dict(its=item(0x10000, 0x10000 + 64, 1.0))):                                  # dlogits inside logits
        assert call(**kw) < 0 and b"uz_lovasz_loss: tensors overlap" in lib.uz_last_error_string(), kw
