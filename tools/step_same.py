#!/usr/bin/env python3
"""Does a change of the Python engine leave every launch and every bit where it was?  For a refactor of engine.py / ops.py, or of
the graphed runners on top of them.

    python tools/step_same.py record OUT.json [--only NAME,...]
    python tools/step_same.py compare A.json B.json [--log-only NAME,...]

`record` runs each configuration below eagerly under ops.profile_begin() and writes, per configuration, the launch log in
order (name, flops, bytes of every timed launch; the 1x1 head, which has no timing bracket, is noted by its route) and the
sha256 of the outputs, the loss, every parameter gradient in named_parameters order and every module buffer after the step.
Run it with the SAME kernel library in both source trees (UNET_ZOO_AMD_LIB); it uses only API that both trees have.
`compare` prints one line per configuration and the first difference, exit status 1 on any; --log-only names configurations
whose numbers differ between two records of ONE tree (compared on their launch log alone, and marked so in the output).

For a refactor of the criteria (criterion.py, loss.py, composed.py, boundary.py, lovasz.py) the criterion/ entries run every
criterion eagerly in its three forms on every output container; there the log is the ordered list of torch operations a
TorchDispatchMode sees around the call and its backward, with the library calls noted through their four entry points."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# tests/test_step_gpu.py::CASES
CASES = [
    ("unet", {}, 2, 64),
    ("attention_unet", {}, 2, 64),
    ("u2net", {}, 2, 64),
    ("swin_unet_v2", {"image_size": 64, "window_size": 4, "drop_path_rate": 0.0}, 2, 64),
    ("nested_unet", {}, 2, 64),
    ("resunet", {}, 2, 64),
    ("missformer", {"image_size": 128}, 2, 128),
    ("transatt_unet", {}, 2, 64),
    ("unet_transformer", {}, 2, 64),
    ("multiresunet", {}, 2, 64),
    ("uctransnet", {"image_size": 64}, 2, 64),
]
EVAL = ("unet", "u2net", "resunet", "vnet", "swin_unet_v2")
FOLDED = ("unet", "attention_unet", "transatt_unet", "nested_unet")
OFF = ("fold_bn_apply", "fold_bn_apply_head", "fold_head_grad", "fold_first_bn_bwd", "fuse_bn_reduce", "direct_first_conv")
SWITCHES = OFF + ("fuse_bn_reduce_convt", "fuse_bn_finalize", "reverse_element_passes", "defer_linear_wgrads", "fold_bn_eval")


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def _tensors(o):
    if isinstance(o, torch.Tensor):
        return [o]
    if isinstance(o, dict):
        return [t for v in o.values() for t in _tensors(v)]
    return [t for v in o for t in _tensors(v)]


def _make(name, kw, dtype, num_classes=1):
    torch.manual_seed(0)
    if name == "missformer":
        from unet_zoo_amd.models import MISSFormer
        m = MISSFormer(num_classes=1, in_channels=3, **kw)
    else:
        m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=num_classes, **kw)
    m.run_dtype = dtype
    for mod in m.modules():          # dropout off: the records compare kernels, not generator states
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.cuda()


def _batch(b, size, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, 3, size, size, generator=g).cuda(), (torch.rand(b, 1, size, size, generator=g) > 0.5).float().cuda())


def folds_batch():
    """the smallest batch at which the 3x3 convolution and its weight gradient read a raw 64-channel 64 x 64 input through
    BatchNorm + ReLU (host-side plan queries)"""
    for n in range(1, 65):
        y = ops.Act(torch.empty((n * 64 * 64, 64), dtype=torch.bfloat16), 0, 64, n, 64, 64)
        if ops.conv_xform_supported(y, 64, 64) and ops.wgrad_xform_shapes_supported(n, 64, 64, 64, 64, 64, 64, torch.bfloat16):
            return n
    raise SystemExit("no batch up to 64 puts a 64 -> 64 channel layer at 64 x 64 on the folded route")


def configs(nf):
    kw = {c[0]: c[1] for c in CASES}
    out = []
    for name, k, b, size in CASES:
        for dt in ("bf16", "fp32"):
            out.append((f"train/{name}/{dt}", dict(model=name, kw=k, b=b, size=size, dtype=dt, mode="train")))
    for name in EVAL:
        for dt in ("bf16", "fp32"):
            out.append((f"eval/{name}/{dt}", dict(model=name, kw=kw.get(name, {}), b=2, size=64, dtype=dt, mode="eval")))
    for dt in ("bf16", "fp32"):
        out.append((f"graphed_eval_fold_bn/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="graphed_eval")))
        out.append((f"frozen_backward/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="frozen")))
        # the graphed runners through their public results (for a refactor of capture.py / step.py / evalstep.py / predict.py / tiled.py)
        out.append((f"graphed_predict/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="graphed_predict")))
        out.append((f"tiled/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="tiled")))
        for crit in ("bce_dice", "callable"):
            out.append((f"graphed_step/{crit}/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="graphed_step", crit=crit)))
    for name in FOLDED:
        out.append((f"folds_on/{name}/bf16/N{nf}", dict(model=name, kw={}, b=nf, size=64, dtype="bf16", mode="train")))
    for s in OFF:
        out.append((f"switch/{s}=False/unet/bf16/N{nf}", dict(model="unet", kw={}, b=nf, size=64, dtype="bf16", mode="train",
                                                               switch={s: False})))
    out.append((f"switch/fuse_bn_finalize=True/unet/bf16/N{nf}", dict(model="unet", kw={}, b=nf, size=64, dtype="bf16", mode="train",
                                                                     switch={"fuse_bn_finalize": True})))
    # the criteria (for a refactor of criterion.py / loss.py / composed.py / boundary.py / lovasz.py): eagerly in their three
    # forms, then inside the graphs of the runners
    for crit in CRITERIA:
        out.append((f"criterion/{crit}", dict(mode="criterion", crit=crit)))
    for crit in ("region", "multiclass", "boundary", "lovasz"):
        for dt in ("bf16", "fp32"):
            out.append((f"graphed_step/{crit}/unet/{dt}", dict(model="unet", kw={}, b=2, size=64, dtype=dt, mode="graphed_step", crit=crit)))
    out.append(("graphed_eval/region/unet/bf16", dict(model="unet", kw={}, b=2, size=64, dtype="bf16", mode="graphed_eval", crit="region")))
    return out


def _take_log():
    log = [[e[0], e[3], e[4]] for e in ops._prof_log]
    ops._prof_log.clear()       # (the head's notes carry no events: profile_end() must not meet them)
    ops.profile_end()
    return log


def _results(sha, tag, obj, names):
    """the sha256 of every tensor in the public result fields `names` of a runner, under tag/"""
    torch.cuda.synchronize()
    for n in names:
        v = getattr(obj, n)
        for i, t in enumerate(_tensors(v) if v is not None else ()):
            sha[f"{tag}/{n}{i}"] = _sha(t)
        if v is None:
            sha[f"{tag}/{n}"] = "none"


def _centre(m, x):
    """move the head's bias so that the logits of x straddle zero: a freshly initialised unet predicts one empty mask"""
    with torch.no_grad():
        bias = [p for n, p in m.named_parameters() if n.endswith("bias") and p.numel() == 1][-1]
        bias -= m(x).float().median()


def run_predict(cfg, m, x, sha):
    """GraphedPredict / SlidingWindowPredict: the results of the capturing call, of a plain replay and of a replay after an in-place
    parameter change; then the launches of one eager pass of the captured pipeline (a capture takes no timing events)"""
    from unet_zoo_amd import MaskPostprocess
    m.eval()
    _centre(m, x)
    if cfg["mode"] == "graphed_predict":
        pred = unet_zoo_amd.GraphedPredict(m, tta=("hflip", "vflip"), postprocess=MaskPostprocess(fill_holes=True, min_area=4))
        names = ("mask", "prob", "labels", "class_map", "stats", "comps", "outputs")
    else:
        x = torch.randn(2, 3, 72, 88, generator=torch.Generator().manual_seed(1)).cuda()
        pred = unet_zoo_amd.SlidingWindowPredict(m, window=(32, 32), overlap=0.5, tile_batch=16, tta=("hflip",))
        names = ("mask", "prob", "labels", "class_map", "stats", "comps")
    for tag in ("first", "second", "changed"):
        if tag == "changed":
            p = next(m.parameters())
            with torch.no_grad():
                p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(9)).cuda())
        pred(x)
        _results(sha, tag, pred, names)
    sha["captures"], sha["describe"] = str(pred.captures), pred.describe()
    ops.profile_begin()
    pred._pipeline(next(iter(pred._graphs.values())))
    return _take_log()


# ------------------------------------------------------------------------------------------------------------- the criteria
CLASSES, IGNORE = 3, 255
CRITERIA = (["bce_dice", "region", "tversky", "ce_dice"] + [f"boundary/{b}" for b in ("bce_dice", "region", "multiclass")]
            + [f"lovasz/{b}/{p}" for b in ("bce_dice", "region", "multiclass") for p in ("per_image", "batch")])
OUTPUT_WEIGHTS = {"tensor": (0.75,), "dict": {"d0": 1.0, "d1": 0.5, "d2": 0.25}, "list": (0.5, 1.0)}
PUBLISHED = ("counts", "term", "sd2", "errors", "ranks")


def _criterion(name, container="tensor"):
    """(the criterion named in CRITERIA / by a graphed entry, whether its targets are class indices); "bce_dice" is a string"""
    from unet_zoo_amd import BoundaryLoss, LovaszLoss, MulticlassLoss, RegionLoss
    parts = name.split("/")
    if parts[0] in ("boundary", "lovasz"):
        base, cls = _criterion(parts[1] if len(parts) > 1 else "region")
        if parts[0] == "boundary":
            return BoundaryLoss(base=base, weight=0.05), cls
        return LovaszLoss(base=base, weight=0.5, per_image=parts[-1] != "batch"), cls
    if name == "bce_dice":
        return "bce_dice", False
    if name == "region":
        return RegionLoss(), False
    if name == "tversky":
        return RegionLoss.tversky(0.6, 0.4, gamma=1.5, reduce="channel", output_weights=OUTPUT_WEIGHTS[container]), False
    if name in ("ce_dice", "multiclass"):
        return MulticlassLoss.ce_dice(class_weight=(0.5, 1.0, 2.0), ignore_index=IGNORE), True
    raise SystemExit(f"no criterion {name!r}")


def _labels(b, h, w, seed):
    """class indices with ignored pixels and ONE value outside [0, CLASSES)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, CLASSES, (b, h, w), generator=g)
    y[torch.rand(b, h, w, generator=g) < 0.1] = IGNORE
    y[0, 1, 2] = CLASSES + 4
    return y


def _op_log(log):
    """a mode under which every torch operation is noted in `log`, in order"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class OpLog(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            log.append([str(func), None, None])
            return func(*args, **(kwargs or {}))
    return OpLog()


def _note_library_calls(log):
    """the four entry points every criterion's kernels are called through, noted in `log` with the number of maps and which of
    them take a gradient; returns what undoes it"""
    from unet_zoo_amd import _lib as L
    saved = [(L, "region_loss"), (L, "class_loss"), (ops, "boundary_loss"), (ops, "lovasz_loss")]
    saved = [(mod, n, getattr(mod, n)) for mod, n in saved]

    def wrap(n, real):
        def call(desc, items, *a):
            log.append(["library:" + n, len(items), "".join("0" if it.dlogits is None else "1" for it in items)])
            return real(desc, items, *a)
        return call
    for mod, n, real in saved:
        setattr(mod, n, wrap(n, real))

    def undo():
        for mod, n, real in saved:
            setattr(mod, n, real)
    return undo


def run_criterion(cfg, sha):
    """one criterion eagerly: loss_and_dice (+ backward), __call__ (+ backward) and direct, on a tensor, a dict of three and a
    list of two, fp32 and bf16 logits; once with a map that needs no gradient and once under no_grad (on tensors that ask for no
    gradient, as GraphedEval hands them over)"""
    from unet_zoo_amd.loss import loss_and_dice, loss_and_dice_direct
    log = []
    undo = _note_library_calls(log)
    cases = [(c, dt, form, "") for c in ("tensor", "dict", "list") for dt in ("fp32", "bf16") for form in ("loss_and_dice", "call", "direct")]
    cases += [("dict", "fp32", "loss_and_dice", "one_map_without_gradient"), ("dict", "bf16", "loss_and_dice", "no_grad")]
    crits = {}
    try:
        for container, dt, form, special in cases:
            if container not in crits:          # (output weights by key go with dict outputs only)
                crits[container] = _criterion(cfg["crit"], container)
            crit, cls = crits[container]
            C = CLASSES if cls else 2
            g = torch.Generator().manual_seed(11)
            n = {"tensor": 1, "dict": 3, "list": 2}[container]
            maps = [(2.0 * torch.randn(2, C, 24, 20, generator=g)).to(torch.bfloat16 if dt == "bf16" else torch.float32).cuda() for _ in range(n)]
            t = _labels(2, 24, 20, 12).cuda() if cls else (torch.rand(2, C, 24, 20, generator=g) > 0.6).float().cuda()
            if special != "no_grad":
                for i, v in enumerate(maps):
                    v.requires_grad_(not (special and i == 1))
            outs = maps[0] if container == "tensor" else ({f"d{i}": v for i, v in enumerate(maps)} if container == "dict" else list(maps))
            tag = "/".join(x for x in (container, dt, form, special) if x)
            log.append(["# " + tag, None, None])
            lad = loss_and_dice if crit == "bce_dice" else crit.loss_and_dice
            with _op_log(log):
                if form == "direct":
                    loss, dice, grads = (loss_and_dice_direct if crit == "bce_dice" else crit.direct)(outs, t)
                elif special == "no_grad":
                    with torch.no_grad():
                        loss, dice = lad(outs, t)
                    grads = ()
                else:
                    if form == "call":
                        loss, dice = (lad(outs, t)[0] if crit == "bce_dice" else crit(outs, t)), None
                    else:
                        loss, dice = lad(outs, t)
                    log.append(["# backward", None, None])
                    loss.backward()
                    grads = [v.grad for v in maps]
            torch.cuda.synchronize()
            sha[tag + "/loss"] = _sha(loss)
            sha[tag + "/dice"] = _sha(dice) if dice is not None else "none"
            for i, gr in enumerate(grads):
                sha[f"{tag}/grad{i}"] = f"{gr.dtype} {_sha(gr)}" if gr is not None else "none"
            for obj, pre in ((crit, ""), (getattr(crit, "base", None), "base.")):
                for name in PUBLISHED:
                    v = getattr(obj, name, None)
                    if isinstance(v, torch.Tensor):
                        sha[f"{tag}/{pre}{name}"] = _sha(v)
    finally:
        undo()
    return log


def backward_seen(log):
    """does the log of a criterion entry hold the multiplication (d * g_loss) of every backward?"""
    backwards = hits = 0
    inside = hit = False
    for name, _, _ in log + [["# end", None, None]]:
        if name.startswith("# "):
            hits += inside and hit
            inside, hit = name == "# backward", False
            backwards += inside
        elif inside and name.startswith("aten.mul"):
            hit = True
    return hits == backwards


def run_step(cfg, m, x, t, sha):
    """GraphedStep: two steps (a composed criterion: a third after set_weights); loss, dice and outputs after each, every
    parameter and buffer after the last"""
    import torch.nn.functional as F
    if cfg["crit"] == "callable":
        crit = lambda o, tt: F.binary_cross_entropy_with_logits(o, tt)      # noqa: E731
    else:
        crit = _criterion(cfg["crit"])[0]
    step = unet_zoo_amd.GraphedStep(m.train(), crit, lr=1e-2)
    for tag in ("first", "second", "reweighted"):
        if tag == "reweighted":
            if not hasattr(crit, "set_weights"):
                break
            crit.set_weights(weight=0.25, base_scale=0.5)
        step(x, t)
        _results(sha, tag, step, ("loss", "dice", "outputs"))
    for n, p in m.named_parameters():
        sha["param/" + n] = _sha(p)
    sha["describe"] = step.describe()
    return []


def run(cfg):
    from unet_zoo_amd.loss import loss_and_dice
    sha = {}
    if cfg["mode"] == "criterion":
        return run_criterion(cfg, sha), sha
    dtype = torch.bfloat16 if cfg["dtype"] == "bf16" else torch.float32
    labels = cfg.get("crit") == "multiclass"
    m = _make(cfg["model"], cfg["kw"], dtype, CLASSES if labels else 1)
    x, t = _batch(cfg["b"], cfg["size"])
    if labels:
        t = _labels(cfg["b"], cfg["size"], cfg["size"], 3).cuda()
    torch.manual_seed(2)
    if cfg["mode"] in ("graphed_predict", "tiled", "graphed_step"):
        log = run_predict(cfg, m, x, sha) if cfg["mode"] != "graphed_step" else run_step(cfg, m, x, t, sha)
        outs = []
    elif cfg["mode"] == "graphed_eval":
        ev = unet_zoo_amd.GraphedEval(m.eval(), _criterion(cfg.get("crit", "bce_dice"))[0], fold_bn=True)
        ops.profile_begin()
        ev._forward(x)                  # the launches of the captured forward, eagerly (a capture takes no timing events)
        log = _take_log()
        loss, dice = ev(x, t)
        torch.cuda.synchronize()
        outs = _tensors(ev.outputs)
        sha["loss"], sha["dice"] = _sha(loss), _sha(dice)
        sha["layers"] = f"{ev.folded_layers} folded, {ev.unfolded_layers} unfolded"
        for tag in ("second", "changed"):       # a plain replay, and one after an in-place parameter change
            if tag == "changed":
                p = next(m.parameters())
                with torch.no_grad():
                    p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(9)).cuda())
            ev(x, t)
            _results(sha, tag, ev, ("loss", "dice", "outputs"))
        sha["describe"] = ev.describe()
    elif cfg["mode"] == "eval":
        m.eval()
        ops.profile_begin()
        with torch.no_grad():
            outs = _tensors(m(x))
        log = _take_log()
    else:
        m.train() if cfg["mode"] == "train" else m.eval()
        ops.profile_begin()
        o = m(x)
        loss = loss_and_dice(o, t)[0]
        loss.backward()
        log = _take_log()
        outs = _tensors(o)
        sha["loss"] = _sha(loss)
        for n, p in m.named_parameters():
            sha["grad/" + n] = _sha(p.grad) if p.grad is not None else "none"
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        sha[f"out{i}"] = _sha(o)
    for n, b in m.named_buffers():
        sha["buf/" + n] = _sha(b)
    return log, sha


def folded_routes(log):
    """which of the three folded routes a launch log shows: the 3x3 convolution, its weight gradient, the 1x1 head"""
    names = [e[0] for e in log]
    return {"conv_igemm _xf": any(n.endswith("_xf") and not n.startswith("wgrad") for n in names),
            "wgrad _xf": any(n.endswith("_xf") and n.startswith("wgrad") for n in names),
            "outconv xform": "outconv_fwd_xf" in names}


def record(path, only):
    defaults = {k: getattr(Engine, k) for k in SWITCHES}
    fwd, bwd = ops.outconv_fwd, ops.outconv_bwd

    def note(name):
        if ops._prof_on:
            ops._prof_log.append((name, None, None, 0.0, 0.0, None))

    def outconv_fwd(x, w, b, xform=None):
        note("outconv_fwd_xf" if xform is not None else "outconv_fwd")
        return fwd(x, w, b, xform=xform)

    def outconv_bwd(x, w, g, dx, dw=None, db=None, bnred=None, lazy=False, store_dx=True):
        note("outconv_bwd" + ("_bnred" if bnred is not None else "") + ("_lazy" if lazy else "") + ("" if store_dx else "_nodx"))
        return bwd(x, w, g, dx, dw, db, bnred=bnred, lazy=lazy, store_dx=store_dx)

    ops.outconv_fwd, ops.outconv_bwd = outconv_fwd, outconv_bwd
    nf = folds_batch()
    res = {"folds_batch": nf, "configs": []}
    for name, cfg in configs(nf):
        if only and not any(o in name for o in only):
            continue
        for k, v in defaults.items():
            setattr(Engine, k, v)
        for k, v in cfg.get("switch", {}).items():
            setattr(Engine, k, v)
        log, sha = run(cfg)
        print(f"{name}: {len(log)} launches", flush=True)
        if name.startswith("folds_on/unet/"):
            missing = [k for k, v in folded_routes(log).items() if not v]
            if missing:
                raise SystemExit(f"{name} does not cover the folded routes: no {', '.join(missing)} launch")
        res["configs"].append({"name": name, "log": log, "sha": sha})
    for k, v in defaults.items():
        setattr(Engine, k, v)
    with open(path, "w") as f:
        json.dump(res, f)


def compare(pa, pb, log_only):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    print(f"batch of the folded entries: N = {a['folds_batch']}")
    seen = [backward_seen(c["log"]) for r in (a, b) for c in r["configs"] if c["name"].startswith("criterion/")]
    if seen:
        print("criterion entries: the log is the torch operations and library calls; the backward's mul is "
              + ("in every log" if all(seen) else "NOT in the log (the gradients' sha256 cover the backward)"))
    if a["folds_batch"] != b["folds_batch"] or [c["name"] for c in a["configs"]] != [c["name"] for c in b["configs"]]:
        print("the two records hold different configurations")
        return 1
    for ca, cb in zip(a["configs"], b["configs"]):
        name, what = ca["name"], None
        if len(ca["log"]) != len(cb["log"]):
            what = f"{len(ca['log'])} launches against {len(cb['log'])}"
        for i, (ea, eb) in enumerate(zip(ca["log"], cb["log"])):
            if ea != eb:
                what = f"launch {i}: {ea} against {eb}"
                break
        if what is None and name not in log_only:
            what = next((f"{k}: {ca['sha'].get(k)} against {cb['sha'].get(k)}" for k in list(ca["sha"]) + list(cb["sha"])
                         if ca["sha"].get(k) != cb["sha"].get(k)), None)
        routes = ""
        if name.startswith("folds_on/unet/"):
            routes = "  [" + ", ".join(k for k, v in folded_routes(ca["log"]).items() if v) + "]"
        tag = "equal (launch log only)" if name in log_only else "equal"
        print(f"{name:58s} {len(ca['log']):5d} launches  {tag if what is None else 'DIFFERENT: ' + what}{routes}")
        bad += what is not None
    print(f"{len(a['configs']) - bad} of {len(a['configs'])} configurations equal")
    return 1 if bad else 0


def _names(argv, flag):
    return argv[argv.index(flag) + 1].split(",") if flag in argv else []


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        import torch
        import unet_zoo_amd
        from unet_zoo_amd import ops
        from unet_zoo_amd.engine import Engine
        record(sys.argv[2], _names(sys.argv, "--only"))
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], _names(sys.argv, "--log-only")))
    else:
        sys.exit(__doc__)
