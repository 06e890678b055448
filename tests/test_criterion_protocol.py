"""The FusedCriterion protocol (criterion.py) without a GPU: a toy criterion whose ``_launch`` is a few torch operations on CPU
tensors shows what the base class promises every criterion -- one ``_launch`` and one autograd node for all output maps,
gradients cast back to each map's dtype, ``need`` following ``requires_grad``, the main map of every container, the
``direct`` form, the output weights, the plan cache -- and what the graphed runners recognise as a criterion."""
import pytest
import torch

from unet_zoo_amd import BoundaryLoss, LovaszLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd.capture import resolve_criterion
from unet_zoo_amd.criterion import INT_DTYPES, FusedCriterion, maps_of

SHAPE = (2, 1, 3, 5)


class Toy(FusedCriterion):
    """loss = sum_m w_m * sum(x_m * target); d(loss)/d(x_m) = w_m * target, in fp32"""
    _NAME = "Toy"

    def __init__(self, output_weights=None):
        super().__init__()
        self.output_weights = self._output_weights(output_weights)
        self.calls, self.built = [], []

    def _build_plan(self, n_items, shape, device, main):
        self.built.append((n_items, tuple(shape), device, main))
        return object()

    def _launch(self, logits, target, weights, main, need):
        self.calls.append((len(logits), tuple(need), main, tuple(weights)))
        self._plan(len(logits), target.shape, target.device, main)
        xs = [v.detach().float() for v in logits]
        loss = sum(w * (x * target).sum() for x, w in zip(xs, weights))
        dice = (xs[main] > 0).float().mean()
        return loss, dice, [w * target.clone() if g else None for w, g in zip(weights, need)]


def _leaf(seed, dtype=torch.float32, grad=True):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(SHAPE, generator=g).to(dtype).requires_grad_(grad)


def _target():
    return torch.rand(SHAPE, generator=torch.Generator().manual_seed(99))


def test_one_launch_and_one_node_for_a_dict_of_three():
    crit, t = Toy(), _target()
    outs = {"d0": _leaf(0), "d1": _leaf(1), "d2": _leaf(2)}
    loss, dice = crit.loss_and_dice(outs, t)
    assert len(crit.calls) == 1 and crit.calls[0] == (3, (True, True, True), 0, (1.0, 1.0, 1.0))
    assert loss.grad_fn is not None and len(loss.grad_fn.next_functions) >= 3
    # ONE node: every leaf's accumulator hangs on the node of the loss itself
    leaves = {id(v) for v in outs.values()}
    assert {id(f.variable) for f, _ in loss.grad_fn.next_functions if f is not None} == leaves
    assert not dice.requires_grad
    loss.backward()
    assert len(crit.calls) == 1                    # the backward launches nothing
    for v in outs.values():
        assert torch.equal(v.grad, t)
    assert torch.equal(crit(outs, t), loss.detach()) and len(crit.calls) == 2      # __call__: the loss alone


def test_a_bf16_leaf_receives_a_bf16_gradient():
    crit, t = Toy(output_weights=[0.5, 2.0]), _target()
    a, b = _leaf(0, torch.bfloat16), _leaf(1)
    loss, _ = crit.loss_and_dice([a, b], t)
    (loss * 3.0).backward()
    g = torch.tensor(3.0)
    assert a.grad.dtype == torch.bfloat16 and torch.equal(a.grad, ((0.5 * t) * g).to(torch.bfloat16))
    assert b.grad.dtype == torch.float32 and torch.equal(b.grad, (2.0 * t) * g)


def test_need_follows_requires_grad():
    crit, t = Toy(), _target()
    a, b = _leaf(0), _leaf(1, grad=False)
    loss, _ = crit.loss_and_dice([a, b], t)
    assert crit.calls[-1][1] == (True, False)
    loss.backward()
    assert a.grad is not None and b.grad is None


def test_under_no_grad_every_need_is_false():
    crit, t = Toy(), _target()
    with torch.no_grad():
        loss, _ = crit.loss_and_dice({"a": _leaf(0), "b": _leaf(1)}, t)
    assert crit.calls[-1][1] == (False, False) and loss.grad_fn is None


def test_main_map_of_every_container():
    crit, t = Toy(), _target()
    crit.loss_and_dice({"a": _leaf(0), "b": _leaf(1), "c": _leaf(2)}, t)
    crit.loss_and_dice([_leaf(0), _leaf(1), _leaf(2)], t)
    crit.loss_and_dice((_leaf(0), _leaf(1)), t)
    crit.loss_and_dice(_leaf(0), t)
    assert [c[2] for c in crit.calls] == [0, 2, 1, 0]
    x = _leaf(0)
    assert maps_of(x) == (None, (x,), 0)
    assert maps_of({"p": 1, "q": 2}) == (("p", "q"), (1, 2), 0) and maps_of([1, 2, 3]) == (None, (1, 2, 3), 2)


def test_direct_returns_the_gradients_in_emission_order():
    crit, t = Toy(output_weights={"b": 2.0, "a": 1.0, "c": 3.0}), _target()
    outs = {"a": _leaf(0), "b": _leaf(1, grad=False), "c": _leaf(2, torch.bfloat16)}
    with torch.no_grad():
        loss, dice, grads = crit.direct(outs, t)
    assert crit.calls == [(3, (True, True, True), 0, (1.0, 2.0, 3.0))]
    assert isinstance(grads, tuple) and len(grads) == 3 and loss.grad_fn is None
    for g, w in zip(grads, (1.0, 2.0, 3.0)):
        assert g.dtype == torch.float32 and torch.equal(g, w * t)
    want, _ = Toy(output_weights=[1.0, 2.0, 3.0]).loss_and_dice(list(outs.values()), t)
    assert torch.equal(loss, want.detach())


def test_weights_for_by_key_and_by_position():
    d = {"a": torch.zeros(1), "b": torch.zeros(1)}
    assert Toy().weights_for(d) == (1.0, 1.0) and Toy().weights_for(torch.zeros(1)) == (1.0,)
    assert Toy(output_weights={"b": 2, "a": 0.5, "z": 9}).weights_for(d) == (0.5, 2.0)
    assert Toy(output_weights=[3, 4]).weights_for(d) == (3.0, 4.0)
    assert Toy(output_weights=(3, 4)).weights_for([d["a"], d["b"]]) == (3.0, 4.0)
    with pytest.raises(ValueError, match=r"Toy: output_weights has no entry for the outputs \['b'\]"):
        Toy(output_weights={"a": 1.0}).weights_for(d)
    with pytest.raises(ValueError, match="Toy: output_weights is a dict but the outputs are not"):
        Toy(output_weights={"a": 1.0}).weights_for([d["a"]])
    with pytest.raises(ValueError, match="Toy: 3 output_weights for 2 output maps"):
        Toy(output_weights=[1, 2, 3]).weights_for(d)
    with pytest.raises(ValueError, match="Toy: output_weights must be >= 0"):
        Toy(output_weights=[1, -2])
    with pytest.raises(ValueError, match=r"Toy: output_weights\['a'\] must be a number"):
        Toy(output_weights={"a": "x"})
    with pytest.raises(ValueError, match=r"Toy: output_weights\[1\] must be finite"):
        Toy(output_weights=[1, float("nan")])


def test_plan_is_built_once_per_key():
    crit, dev = Toy(), torch.device("cpu")
    p = crit._plan(2, SHAPE, dev, 1)
    assert crit._plan(2, torch.Size(SHAPE), dev, 1) is p and len(crit.built) == 1
    for key in ((3, SHAPE, dev, 1), (2, SHAPE[:3] + (6,), dev, 1), (2, SHAPE, dev, 0), (2, SHAPE, torch.device("cuda", 1), 1)):
        assert crit._plan(*key) is not p       # (a device is only named here: the base class touches no GPU API)
        crit._plan(*key)
    assert len(crit.built) == 5 and crit.built[-1][2].index == 1
    with pytest.raises(NotImplementedError):
        FusedCriterion()._plan(1, SHAPE, dev, 0)


def test_the_base_class_settings():
    assert FusedCriterion.target_dtype == torch.float32 and Toy().target_dtype == torch.float32
    assert torch.int32 in INT_DTYPES and torch.float32 not in INT_DTYPES and torch.bool not in INT_DTYPES
    for c in (RegionLoss(), MulticlassLoss(), BoundaryLoss(), LovaszLoss()):
        assert isinstance(c, FusedCriterion) and c._NAME == type(c).__name__


@pytest.mark.parametrize("make", [RegionLoss, MulticlassLoss, BoundaryLoss, lambda: BoundaryLoss(base=MulticlassLoss()), LovaszLoss,
                                  lambda: LovaszLoss(base=MulticlassLoss()), Toy, lambda: "bce_dice", lambda: (lambda o, t: 0)],
                         ids=["RegionLoss", "MulticlassLoss", "BoundaryLoss", "BoundaryLoss-class", "LovaszLoss", "LovaszLoss-class",
                              "toy", "bce_dice", "callable"])
def test_resolve_criterion_returns_a_fused_pair(make):
    from unet_zoo_amd.loss import loss_and_dice, loss_and_dice_direct
    c = make()
    fused, dtype = resolve_criterion(c)
    if isinstance(c, str):
        assert fused == (loss_and_dice, loss_and_dice_direct) and dtype == torch.float32
    elif isinstance(c, FusedCriterion):
        assert fused == (c.loss_and_dice, c.direct) and dtype == c.target_dtype
    else:
        assert fused is None and dtype == torch.float32
