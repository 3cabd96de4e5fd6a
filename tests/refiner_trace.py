"""A recorder for the refiner's launch sequence and the configurations tests/test_refiner_trace_gpu.py pins with it: every public launching
function of `ops` that VolumeRefiner.run_feature_net, feature_volumes and run_volume_net reach is wrapped by attribute (nested calls — the
affine_split16 pass inside ops.conv's variant 5 — are seen too) and each call is written down as [name, {parameter: description}, result].
A tensor is its shape, dtype, strides, storage offset and the ordinal of its storage in first-seen order (the recorder keeps every tensor
it meets alive, so no storage is reused and the ordinals follow from the call order alone: about 2 GB at four volumes); a PairMap is its
tensor plus its slot's name; a (RangeTable, slot[, variant]) argument is the slot's name (and variant).  An argument of a type that is not
listed here raises: nothing is skipped.  The outputs' values are not compared (the InstanceNorm sums are fp64 atomics)."""
import contextlib
import inspect

import torch

from gen6d_amd import ops, synth
from test_networks_gpu import _net
from test_refiner_volume_pairs_gpu import _features

WRAPPED = ("conv", "conv16_direct_multi", "affine_split16", "affine_split16_to", "upsample_bilinear_split16", "l2norm_split16", "l2norm_rows",
           "affine_act_pool", "upsample_bilinear", "new_map16", "new_stats", "stats_finalize", "refiner_volume_kp", "refiner_volume_kp_pairs",
           "fork_join",
           # the trunk's entry points (backbone.vgg_taps_cl / vgg_taps_cl_multi / _vgg_taps_conv16)
           "vgg_conv1_pool_nhwc", "vgg_conv1_pool_nhwc16", "wino_conv3x3", "wino_conv3x3_multi", "wino43_conv3x3_multi", "wino16_conv3x3_multi",
           "alloc_like_segments")


class Recorder:
    def __init__(self):
        self.trace, self.keep, self.storages = [], [], {}

    def tensor(self, t):
        self.keep.append(t)
        key = t.untyped_storage().data_ptr()
        ordinal = self.storages.setdefault(key, len(self.storages))
        return {"shape": list(t.shape), "dtype": str(t.dtype), "strides": list(t.stride()), "offset": t.storage_offset(), "storage": ordinal}

    @staticmethod
    def slot_name(table, slot):
        return next(n for n, i in table.names.items() if i == slot)

    def describe(self, v):
        if torch.is_tensor(v):
            return self.tensor(v)
        if isinstance(v, ops.PairMap):
            return {"pairs": self.tensor(v.data), "slot": self.slot_name(v.table, v.slot)}
        if isinstance(v, ops.Conv16Filters):
            return {"filters": self.tensor(v.data), "layout": v.layout, "mode": v.mode, "acc_scale": v.acc_scale, "Cout": v.Cout, "taps": v.taps,
                    "Cin": v.Cin}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        if isinstance(v, (list, tuple)):
            if v and isinstance(v[0], ops.RangeTable):          # rng = (table, slot) / pairs = (table, slot[, variant])
                return {"slot": self.slot_name(v[0], v[1]), **({"variant": int(v[2])} if len(v) == 3 else {})}
            return [self.describe(x) for x in v]
        raise TypeError(f"refiner_trace: cannot describe an argument of type {type(v).__name__}")

    def wrap(self, name):
        fn = getattr(ops, name)
        sig = inspect.signature(fn)

        def recorded(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()                             # the call as the op sees it, however its arguments were passed
            if name == "fork_join":                            # its branches are closures: their number; their launches follow as calls
                args = {"fns": len(bound.arguments["fns"]), "device": str(bound.arguments["device"])}
            else:
                args = {k: self.describe(v) for k, v in bound.arguments.items()}
            entry = [name, args, None]
            self.trace.append(entry)                           # in call order: a nested call follows the call that made it
            out = fn(*a, **kw)
            entry[2] = self.describe(out)
            return out
        return recorded

    @contextlib.contextmanager
    def installed(self):
        saved = {n: getattr(ops, n) for n in WRAPPED}
        try:
            for n in WRAPPED:
                setattr(ops, n, self.wrap(n))
            yield self
        finally:
            for n, fn in saved.items():
                setattr(ops, n, fn)


def _crops(n, size):
    c = synth.refiner_case()
    imgs = torch.cat([c["ref_imgs"][0], c["que_imgs"]], 0)                       # the seven crops of one step, query last
    return imgs.repeat(n // 7, 1, 1, 1)[..., :size, :size].contiguous().cuda()


def _volume(net, qn):
    args = _features(max(qn, 1))
    if qn == 0:                                                                  # one unbatched query
        args = tuple(a[0] for a in args)
    ops.stats_arena_begin(args[0].device)
    mean_in, std = net.feature_volumes(*args, 128, 128, 32)
    net.run_volume_net(mean_in, std, 32)


def _featnet(net, n, size, **kw):
    imgs = _crops(n, size)
    ops.stats_arena_begin(imgs.device)
    net.run_feature_net(imgs, **kw)


# name -> (network cfg, forced routes (a name the caller's `forcing` understands, or None), run(net))
CONFIGS = {
    "volume.single": ({}, None, lambda net: _volume(net, 0)),
    "volume.4": ({}, None, lambda net: _volume(net, 4)),
    "volume.4.fp32_cores": ({"fp32_cores": True}, None, lambda net: _volume(net, 4)),
    "volume.4.fp16": ({"math_mode": "fp16"}, None, lambda net: _volume(net, 4)),
    "volume.4.fp16.keep_stack_tail": ({"math_mode": "fp16", "lowp_keep_fp32": ("stack", "tail")}, None, lambda net: _volume(net, 4)),
    "volume.4.embeds_only": ({}, "embeds_only", lambda net: _volume(net, 4)),
    "volume.4.igemm_variant3": ({}, "igemm_variant3", lambda net: _volume(net, 4)),
    "featnet.7": ({}, None, lambda net: _featnet(net, 7, 128)),
    "featnet.28": ({}, None, lambda net: _featnet(net, 28, 128)),
    "featnet.28.fp32_cores": ({"fp32_cores": True}, None, lambda net: _featnet(net, 28, 128)),
    "featnet.28.fp16": ({"math_mode": "fp16"}, None, lambda net: _featnet(net, 28, 128)),
    "featnet.28.f43_false": ({}, None, lambda net: _featnet(net, 28, 128, f43=False)),
    "featnet.28.conv_out_only": ({}, "conv_out_only", lambda net: _featnet(net, 28, 128)),
    "featnet.28.96x96": ({}, None, lambda net: _featnet(net, 28, 96)),
}


def record(name, forcing):
    """Run configuration `name` under the recorder -> {"trace", "labels" (ops.PROFILE), "slots" (range_report's keys)}.  forcing(name) is
    the caller's context manager that forces the named routes (the module constants at the parent, the route table since)."""
    cfg, forced, run = CONFIGS[name]
    with (forcing(forced) if forced else contextlib.nullcontext()):
        net = _net("refiner", **cfg)
        rec = Recorder()
        ops.PROFILE = []
        try:
            # cfg 'math_mode' is applied by _step: the same context round the parts that are called directly here
            with torch.no_grad(), ops.math_mode(net.cfg.get("math_mode"), inherit_if_none=True), rec.installed():
                run(net)
            torch.cuda.synchronize()
            labels = [e[3] for e in ops.PROFILE]
        finally:
            ops.PROFILE = None
    return {"trace": rec.trace, "labels": labels, "slots": sorted(net.range_report())}
