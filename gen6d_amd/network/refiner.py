"""VolumeRefiner — drop-in for the reference's network/refiner.py (same constructor, state_dict keys, forward dict).

One refinement step (reference forward, refiner.py:249-269):
    own channels-last Winograd trunk (backbone.py) on the 6 reference crops + the query crop, g6d_l2norm_rows on its taps
    RefineFeatureNet 2-D convs on g6d_conv_igemm; every InstanceNorm2d is a per-image (sum, sumsq) epilogue of the
        producing conv and an affine(+ReLU) in the loader of the consuming conv / up-sampler      refiner.py:24-51,64-78
        (batched calls of the fp32 path: on fp16 hi / lo pairs, g6d_conv16_direct_multi with g6d_l2norm_split16, g6d_affine_split16 and
        the slice producers g6d_affine_split16_to / g6d_upsample_bilinear_split16 as hand-over passes — the "pair" entries of ROUTES)
    g6d_refiner_volume: projection + bilinear sampling + mean/std over references, fused            refiner.py:183-247
    RefineVolumeEncodingNet 3x3x3 convs on g6d_conv_igemm (32^3 layers: Winograd F(4x4,3x3), depth taps folded into the reduction;
        16^3: F(2x2,3x3); 8^3/4^3 and stride-2 layers: implicit 3-D GEMM with split-K — in batched calls of the fp32 path the "igemmV"
        entries of ROUTES in that kernel's own fp16 hi / lo pair mode)
        (batched calls of the fp32 path: the "pair" entries of ROUTES on fp16 hi / lo pairs, g6d_conv16_direct_multi with
        depth-folded filters; g6d_refiner_volume_kp_pairs writes their input volumes as pairs)
Both nets are ONE layer table each (FEATNET, VOLUME) walked by _run_net; which kernel a layer takes in the big calls of the fp32 path is
ONE table (ROUTES), resolved per call by resolve_routes.
    g6d_linear_gemv_batch: the 32768->512 FC is a 67 MB weight stream, read once per 8 queries                                    refiner.py:153-166
"""
import itertools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops, specs
from .backbone import pack_trunk, trunk_features
from .operator import pose_apply_th
from .params import ParamBank, fold_vgg

# Winograd F(4x4,3x3) (csrc/wino43_conv.hip) for the crops' VGG trunk (1.31-1.35x over F(2x2,3x3) at 56 crops, profiles/r04_w43_bench_v5.md;
# on the fp32 path the trunk then runs on fp16 hi / lo pairs, backbone.trunk_route) and the layers that list "f43" in ROUTES.
# All of it pays from ~4 queries per launch on: one query's 7 crops / single volume leave most CUs without a block and the kernel's longer
# per-block prologue / epilogue shows (measured per step at batch 1: crops' trunk 475 vs 320 us, volume layers 541 vs 418 us on
# F(2x2,3x3); at batch 8: 1.06 vs 1.43 ms and 1.96 vs 3.06 ms the other way round)
F43_MIN_QUERIES = 4
MAX_BATCH = 32         # queries that share one set of launches (g6d_linear_gemv_batch: 8 right-hand sides per weight pass)


class Layer(NamedTuple):
    """One 3x3 / 3x3x3 layer of the refiner, declared once: _pack, the route plan, the run functions and the per-layer tools
    (tools/*_layers.py) read names and shapes from here.  `key` also names the layer in ROUTES and prefixes its range slots."""
    key: str
    weights: str             # its prefix in the state dict; the packed filters sit under `key` in _pack()
    cin: int
    cout: int
    stride: int
    div: int                 # its input map's edge: the call's size // div
    norm: bool               # an InstanceNorm follows: statistics in the epilogue + finalize, handed on as an affine
    part: str                # the part of _mm it belongs to
    src: str = None          # the named map it reads (an input volume, a trunk tap, `cat`; also that map's range slot); None: the layer before it
    dst: tuple = None        # a branch's last layer: (channel offset in `cat`, up-sampling factor)

    # depth taps: the feature net's layers are (1,3,3), the volume net's (3,3,3)
    kd = property(lambda self: 1 if self.part == "featnet" else 3)
    # packs F(2x2,3x3) filters (the 8^3 -> 4^3 tail never runs on the Winograd kernel)
    wino = property(lambda self: self.stride == 1 and self.part != "tail")
    # what the halo-patch kernel cannot express (stride 2, or maps small enough to need split-K): a candidate of the implicit-GEMM pair mode
    igemm = property(lambda self: self.kd == 3 and (self.stride == 2 or self.div >= 4))
    # range slot of the hand-over pass in front of it (names pinned by range_report's readers)
    pass_slot = property(lambda self: self.key[:-2] + ".mid" if self.key.endswith(".3") else self.key + ".in")

    def edge(self, size, out=False):
        """Its input (out: output) map's extents for a call of `size` ((h, w) crops, (sn, sn, sn) volumes)."""
        return tuple(s // (self.div * (self.stride if out else 1)) for s in size)


class Net(NamedTuple):
    name: str
    layers: tuple
    together: bool           # the layers that list "pair" take the pair kernel together or not at all (see resolve_routes)
    align: int               # the pair routes need crop sizes that are multiples of it

    def layer(self, key):
        return next(L for L in self.layers if L.key == key)

    def reader(self, src):
        return next(L for L in self.layers if L.src == src)

    def chains(self):
        """The layers in runs that start at a named map: the branches that end in `cat`, then the chain that reads it."""
        out = []
        for L in self.layers:
            if L.src:
                out.append([])
            out[-1].append(L)
        return out


def _branch(net, name, cin, cmid, cout, div, part, src, dst=None):
    """A conv, IN, ReLU, conv branch (the Sequential's layers 0 and 3); a join into `cat` takes the second layer's own InstanceNorm along."""
    tree = "feature_net" if net == "featnet" else "volume_net"
    return (Layer(f"{net}.{name}.0", f"{tree}.{name}.0", cin, cmid, 1, div, True, part, src=f"{net}.{src}"),
            Layer(f"{net}.{name}.3", f"{tree}.{name}.3", cmid, cout, 1, div, net == "featnet", part, dst=dst))


def _stack(name, cin, cout, stride, div, part="stack", norm=True, src=None):
    return Layer(f"volume.{name}", f"volume_net.{name if '.' in name else name + '.0'}", cin, cout, stride, div, norm, part, src=src)


FEATNET = Net("featnet", (*_branch("featnet", "conv0", 256, 64, 64, 4, "featnet", "f3", (0, 1)),
                          *_branch("featnet", "conv1", 512, 256, 64, 8, "featnet", "f5", (64, 2)),
                          *_branch("featnet", "conv2", 512, 256, 64, 16, "featnet", "f7", (128, 4)),
                          *_branch("featnet", "conv_out", 192, 128, 128, 4, "featnet", "cat")), together=False, align=16)
VOLUME = Net("volume", (*_branch("volume", "mean_embed", 256, 64, 64, 1, "embed", "mean_in", (0, 1)),
                        *_branch("volume", "var_embed", 128, 64, 64, 1, "embed", "std", (64, 1)),
                        _stack("conv0", 128, 64, 1, 1, src="volume.cat"), _stack("conv1", 64, 128, 2, 1), _stack("conv2", 128, 128, 1, 2),
                        _stack("conv3", 128, 256, 2, 2), _stack("conv4", 256, 256, 1, 4), _stack("conv5.0", 256, 512, 2, 4, "tail"),
                        _stack("conv5.3", 512, 512, 1, 8, "tail", norm=False)), together=True, align=1)

# layer -> its routes in the big calls (from F43_MIN_QUERIES queries) of the fp32 path, in order of preference; resolve_routes turns
# them into the route each layer takes in one call.  A layer that lists none keeps the fp32 cores' F(2x2,3x3) / implicit GEMM.
#   "pair"    the fp16 hi / lo pair kernel (conv16w_kernel<3,.>: fp32-class products on the 16-bit matrix cores; 3x3x3 layers with their
#             depth taps folded into the reduction, filter layout 2), its input handed over as a PairMap.  Feature net: per branch at
#             112 crops, hand-over passes included, all four faster (tools/featnet_layers.py, profiles/r16_featnet_pairs.md).  Volume
#             net: per layer at 16 volumes (tools/volume_layers.py, profiles/r17_volume_pairs.md): embeds 1675 -> 1308 and 1093 -> 833 us,
#             conv0 642 -> 512, conv2 294 -> 128
#   "igemmV"  the implicit-GEMM kernel's own pair mode with loader variant V (ops.conv(pairs=(table, slot, V))): 3 = both operands split
#             in the loader, 4 = filters pre-split by the weight pack (bit-identical to 3), 5 = activations pre-split as well by one
#             affine_split16 pass.  Per layer at 16 volumes the fastest variant that beats the layer's route by more than that route's
#             spread (tools/igemm_pair_layers.py, profiles/r18_igemm_pairs.md, profiles/r22_igemm_presplit.md).  conv4 (8^3) competes
#             with F(2x2,3x3) and stays there: a listed layer's label may only gain the `conv16x3 igemm` prefix
#             (tests/test_igemm_pair_routes_gpu.py)
#   "f43"     packs F(4x4,3x3) filters: the fp32 cores' kernel of the big calls that are not on pairs.  Feature net per layer at 56 crops
#             against F(2x2,3x3) (profiles/r04_layer_table_featnet_f43.md): 512->256 @16x16 159 vs 173 us, 192->128 @32x32 119 vs 148,
#             128->128 @32x32 107 vs 129 kept; 256->64 @32x32 131 vs 94, 256->64 @16x16 88 vs 60, 512->256 @8x8 108 vs 80 not.  Volume net:
#             the 32^3 layers 1.4-1.5x (profiles/r04_w43_bench_v5.md); per batch of 8 conv2 (16^3) 147 vs 151 us, conv4 (8^3) 144 vs 94: not
ROUTES = {
    "featnet.conv0.0": ("pair",), "featnet.conv0.3": ("pair",),
    "featnet.conv1.0": ("pair", "f43"), "featnet.conv1.3": ("pair",),
    "featnet.conv2.0": ("pair",), "featnet.conv2.3": ("pair",),
    "featnet.conv_out.0": ("pair", "f43"), "featnet.conv_out.3": ("pair", "f43"),
    "volume.mean_embed.0": ("pair", "f43"), "volume.mean_embed.3": ("pair", "f43"),
    "volume.var_embed.0": ("pair", "f43"), "volume.var_embed.3": ("pair", "f43"),
    "volume.conv0": ("pair", "f43"), "volume.conv1": ("igemm5",), "volume.conv2": ("pair",), "volume.conv3": ("igemm5",),
    "volume.conv4": (), "volume.conv5.0": ("igemm5",), "volume.conv5.3": ("igemm5",),
}


def admission_shapes(net, routes, n, size):
    """{layer: (N, H, W, Cin, Cout, stats_rows, D)}: the questions to ops.conv16_direct_plan for the layers of `net` that list "pair", in a
    call of n maps of `size` — each with statistics groups of whole maps (D: the depth of a 3x3x3 layer's volumes, else None)."""
    out = {}
    for L in net.layers:
        if "pair" in routes.get(L.key, ()):
            *d, h, w = L.edge(size)
            out[L.key] = (n, h, w, L.cin, L.cout, h * w * (d[0] if d else 1), d[0] if d else None)
    return out


def resolve_routes(net, routes, size, big, rng, rng_part, answers):
    """`routes` resolved for one call -> {layer: "pair" | "igemm3" / "igemm4" / "igemm5" | "f43" | "cores"}.
    big: the call is big.  rng: a range table is available where the call's inputs are made (what the pair kernel's layers depend on:
    their inputs exist as pairs from the start).  rng_part: one is available inside the layer's own part of _mm (what the implicit-GEMM
    pair mode depends on: under an outer reduced-precision mode a part kept on fp32 still runs it).  answers: {layer:
    ops.conv16_direct_plan's answer} to admission_shapes.
    "pair" needs big, rng and the halo-patch kernel (answers 1 / 2) for the layer; in the feature net (net.together False) per branch:
    every layer of it, on crops of multiples of net.align; in the volume net all listed layers or none, with both embeds among them
    (g6d_refiner_volume_kp_pairs then writes BOTH input volumes as pairs: they never exist in fp32)."""
    listed = [L for L in net.layers if "pair" in routes.get(L.key, ())]
    fits = lambda ls: all(L in listed and answers.get(L.key) in (1, 2) for L in ls)
    chains = net.chains()
    if not (big and rng) or any(s % net.align for s in size):
        pair = []
    elif net.together:
        pair = listed if fits(listed + [L for c in chains if c[-1].dst for L in c]) else []
    else:
        pair = [L for c in chains if fits(c) for L in c]
    out = {}
    for L in net.layers:
        mine = routes.get(L.key, ())
        igemm = next((r for r in mine if r.startswith("igemm")), None)
        out[L.key] = "pair" if L in pair else igemm if (igemm and big and rng_part) else "f43" if (big and "f43" in mine) else "cores"
    return out


_LIN = {}


def _linspace(sn, dev):
    """torch.linspace(-1, 1, sn) cached per (sn, device): a constant of the configuration, not a launch per step."""
    key = (sn, str(dev))
    if key not in _LIN:
        _LIN[key] = torch.linspace(-1, 1, sn, dtype=torch.float32, device=dev)
    return _LIN[key]


class RefFeatureCache:
    """Features of aligned reference crops ([fh,fw,C] device tensors) keyed by (database, view id, in-plane angle bucket, crop
    size): with `ref_feat_cache_deg` > 0 the alignment angle of a reference view is snapped to that grid, so a (view, bucket) pair
    always yields the same crop and its trunk + feature-net pass (6 of the 7 images of a refinement step) can be skipped when the
    pair repeats — between the refinement steps of a query and between queries (the reference re-warps and
    re-extracts all six views every step, refiner.py:289-313).  LRU-bounded (0.5 MB per entry)."""

    def __init__(self, max_entries=2048):
        from collections import OrderedDict
        self.store, self.max_entries = OrderedDict(), max_entries
        self.hits = self.misses = 0

    def get(self, key):
        f = self.store.get(key)
        if f is None:
            self.misses += 1
            return None
        self.store.move_to_end(key)
        self.hits += 1
        return f

    def put(self, key, feat):
        self.store[key] = feat
        while len(self.store) > self.max_entries:
            self.store.popitem(last=False)

    def clear(self):
        self.store.clear()
        self.hits = self.misses = 0

    @property
    def hit_rate(self):
        return self.hits / max(1, self.hits + self.misses)


class VolumeRefiner(ParamBank):
    # ref_feat_cache_deg: 0 = the reference's exact alignment, nothing cached (default); > 0 = alignment angles snapped to this
    # grid (degrees) and reference-crop features cached per (view, bucket) — opt-in: the snapped angle changes the crops
    # lowp_keep_fp32 / lowp_only: as in ViewpointSelector — parts that stay on fp32 matrix-core operands in the reduced-precision mode:
    # "trunk" (VGG on the crops), "featnet" (the four conv pairs of the 2-D feature net), "embed" (mean_embed / var_embed on the 32^3
    # volume), "stack" (volume_net conv0..conv4), "tail" (conv5 pair on 8^3 / 4^3 maps); lowp_only: ONLY the named parts on 16 bits
    # (tools/lowp_refiner_sensitivity.py)
    default_cfg = {"refiner_sample_num": 32, "ref_feat_cache_deg": 0.0, "lowp_keep_fp32": (), "lowp_only": None}

    def __init__(self, cfg):
        self.cfg = {**self.default_cfg, **cfg}
        super().__init__(specs.refiner_rows())
        self.ref_database = None
        self.ref_ids = None
        self.feat_cache = RefFeatureCache()

    def load_state_dict(self, *a, **k):
        self.feat_cache.clear()                      # cached features belong to the weights they were computed with
        return super().load_state_dict(*a, **k)

    def _mm(self, *names):
        """math-mode context of one part: fp32 if listed in cfg['lowp_keep_fp32'] (with cfg['lowp_only']: if NOT listed there)."""
        only = self.cfg.get("lowp_only")
        keep = self.cfg.get("lowp_keep_fp32") or ()
        fp32 = (not any(n in only for n in names)) if only is not None else any(n in keep for n in names)
        return ops.math_mode("fp32" if fp32 else None, inherit_if_none=True)

    def angle_step(self):
        """Snap grid of the reference alignment in radians (0 = exact, no caching)."""
        return float(np.radians(self.cfg.get("ref_feat_cache_deg") or 0.0))

    def cached_ref_feats(self, keys, make_imgs):
        """Features [len(keys),fh,fw,C] of the reference crops with cache keys `keys`; make_imgs(missing_positions) must return the
        crops [m,3,h,w] in [0,1] of the positions that are not cached (they go through the feature net in one batch)."""
        # features depend on the matrix-core operand precision they were computed in: the mode is part of the key, and misses run in
        # the network's own mode like _step does
        with ops.math_mode(self.cfg.get("math_mode"), inherit_if_none=True):
            keys = [(k, ops.MATH_MODE) for k in keys]
            got = [self.feat_cache.get(k) for k in keys]
            miss = [i for i, f in enumerate(got) if f is None]
            # (f43=False: a cached feature must not depend on how many keys missed together — the F(2x2,3x3) / F(4x4,3x3) choice of
            # run_feature_net follows the batch size otherwise)
            feats = self.run_feature_net(make_imgs(miss), f43=False) if miss else None
        if miss:
            for j, i in enumerate(miss):
                got[i] = feats[j].clone()
                self.feat_cache.put(keys[i], got[i])
        return torch.stack(got, 0)

    # ------------------------------------------------------------------ weights
    def _pack(self):
        if self._packed is None:
            pk = {"vgg": pack_trunk(fold_vgg(self, "feature_net.backbone.features"))}
            for L in FEATNET.layers + VOLUME.layers:
                pk[L.key] = self.conv_w(L.weights, wino_kd=L.kd if L.wino else 0, f43="f43" in ROUTES.get(L.key, ()))
                if L.igemm:
                    # filter exponent and pre-split pack of a layer that may run on the implicit-GEMM pair modes: computed here (a
                    # device-to-host read of max |w|, an allocation), not at its first launch, which may sit inside a graph capture
                    ops.pair_filter_prepare(pk[L.key][0])
                    ops.pair_filter_pack(pk[L.key][0])
            # fc.0.0 consumes x.flatten(1) of [512,4,4,4] (index c*64+v); our code is [v][c] -> permute once
            w = self.p("regressor.fc.0.0.weight")
            pk["fc0"] = (w.reshape(512, 512, 64).permute(0, 2, 1).reshape(512, 32768).contiguous(),
                         self.p("regressor.fc.0.0.bias").contiguous())
            pk["fc1"] = (self.p("regressor.fc.1.0.weight").contiguous(), self.p("regressor.fc.1.0.bias").contiguous())
            heads = ("fcr", "fct", "fcs")
            pk["heads"] = (torch.cat([self.p(f"regressor.{h}.weight") for h in heads], 0).contiguous(),
                           torch.cat([self.p(f"regressor.{h}.bias") for h in heads], 0).contiguous())
            self._packed = pk
        return self._packed

    # ------------------------------------------------------------------ routes, layers, hand-over, join
    def _plan(self, net, n, size, big, rng):
        """ROUTES resolved for a call of `net` on n maps of `size` -> (routes without, routes with a range table inside the layer's own
        part): resolve_routes on the library's admission answers, asked once per (count, size, table content), so that no launch path
        queries the library."""
        key = (net.name, n, size, big, rng, tuple(ROUTES.items()))
        memo = self.__dict__.setdefault("_plans", {})
        if key not in memo:
            ask = admission_shapes(net, ROUTES, n, size) if (big and rng) else {}
            answers = {k: ops.conv16_direct_plan(N, H, W, ci, co, 3, stats_rows=rows, D=D) for k, (N, H, W, ci, co, rows, D) in ask.items()}
            memo[key] = tuple(resolve_routes(net, ROUTES, size, big, rng, part, answers) for part in (False, True))
        return memo[key]

    def run_layer(self, L, route, x, y, aff=None, stats=None):
        """Layer L on `route` (resolve_routes) into the fp32 view y [N,D,H,W,Cout] (a dense map or a channel slice of one; D = 1 in
        2-D).  x: for "pair" the PairMap it reads (planes as images or whole volumes); else the producer's fp32 map, whose InstanceNorm
        affine `aff` (+ ReLU) the launch applies in its operand prologue (a table per map from two maps on; the 2-D net: always).
        stats: the statistics buffer, if the caller took it already.  Returns the affine (scale, shift) of the InstanceNorm that follows
        the layer (sums in the epilogue; finalised by the launch itself or one small launch), or None."""
        w = self._pack()[L.key]
        n, count = y.shape[0], y.shape[1] * y.shape[2] * y.shape[3]
        st = stats if stats is not None else ops.new_stats(n, L.cout, y.device) if L.norm else None
        if route == "pair":
            ops.conv16_direct_multi([x.view(*y.shape[:4], 2, L.cin) if L.kd == 3 else x], w.w16(3, layout=2 if L.kd == 3 else 1), w[1], relu=False,
                                    full=torch.float32, kd=L.kd, stats=st, rows_per_group=count if L.norm else 0, out_full=[y if L.kd == 3 else y[:, 0]])
            return ops.stats_finalize(st, count) if L.norm else None
        if route.startswith("igemm"):       # under the layer's own slot: no hand-over pass but the one variant 5 makes itself
            table = self.range_table()
            kernel = {"pairs": (table, table.slot(L.key + ".igemm"), int(route[5:]))}
        else:
            kernel = {"w_wino": w.u, "w_wino43": w.u43 if route == "f43" else None}
        pn = 1 if (n > 1 or L.kd == 1) else 0
        sc, sh = aff or (None, None)
        out = ops.conv(x, w[0], w[1], y, ksize=(L.kd, 3, 3), stride=(L.stride if L.kd == 3 else 1, L.stride, L.stride), pad=(L.kd // 2, 1, 1),
                       in_scale=sc, in_shift=sh, in_relu=aff is not None, per_n=pn if aff is not None else 0, stats=st,
                       rows_per_group=pn * count if L.norm else 0, finalize=count if L.norm else None, **kernel)
        return out if L.norm else None

    def to_pairs(self, y, aff, slot):
        """THE hand-over pass: the fp32 map y [N,D,H,W,C] behind its producer's InstanceNorm affine `aff` + ReLU (None: as it is) -> the
        PairMap a layer on the pair kernel reads, under range slot `slot` (planes as images: D planes per affine table)."""
        table = self.range_table()
        sc, sh = aff or (None, None)
        return ops.affine_split16(y.view(-1, 1, *y.shape[2:]), sc, sh, y.shape[1] if aff is not None else 0, aff is not None, False, 3,
                                  rng=(table, table.slot(slot)))

    @staticmethod
    def join(y, aff, cat, c_off, factor):
        """THE join: a branch's fp32 map y [N,D,H,W,C] behind its InstanceNorm affine `aff` (None: as it is; no ReLU), up-sampled by
        `factor`, into channels [c_off, c_off + C) of `cat` — an fp32 map or a PairMap (whose slices share ONE exponent slot)."""
        sc, sh = aff or (None, None)
        if isinstance(cat, ops.PairMap):
            planes, per = y.view(-1, 1, *y.shape[2:]), y.shape[1] if aff is not None else 0
            if factor == 1:
                ops.affine_split16_to(planes, sc, sh, per, False, 3, cat, c_off)
            else:
                ops.upsample_bilinear_split16(planes, cat, c_off, factor, sc, sh, per, 3)
        elif factor == 1:
            ops.affine_act_pool(y, cat[..., c_off:c_off + y.shape[-1]], sc, sh, per_n=True)
        else:
            ops.upsample_bilinear(y, cat[..., c_off:c_off + y.shape[-1]], factor, sc, sh, per_n=True)

    def _run_net(self, net, maps, n, size, big, rng, dev, fork):
        """The walk over `net`'s layer table for n maps of `size`: each chain reads its named map of `maps` (a function of whether the
        reader takes pairs, where the two differ), every layer runs on its resolved route (run_layer), and a layer on the pair kernel
        whose producer left an fp32 map gets it through to_pairs; the branches meet in `cat` — a PairMap when its reader runs on the pair
        kernel, else fp32 — through join, or by writing their slice themselves where there is nothing to apply.  rng: whether the call's
        inputs were made with a range table; fork: the branches run as parallel launch sequences.  -> the last layer's (map, affine)."""
        plan = self._plan(net, n, size, big, rng)
        reader = net.reader(net.name + ".cat")
        lead = lambda e: (n, *((1,) if len(e) == 2 else ()), *e)
        if plan[0][reader.key] == "pair":
            table, e = self.range_table(), reader.edge(size)
            cat = ops.new_map16(n * (e[0] if len(e) == 3 else 1), e[-2], e[-1], reader.cin, 3, dev, rng=(table, table.slot(reader.src)))
        else:
            cat = torch.empty((*lead(reader.edge(size)), reader.cin), dtype=torch.float32, device=dev)
        maps = {**maps, reader.src: cat}

        def run(chain):
            pairs = plan[0][chain[0].key] == "pair"            # (the pair kernel's routes do not depend on the part)
            y, aff = maps[chain[0].src], None
            if callable(y):
                y = y(pairs)
            # (the 2-D net takes a chain's statistics in front of its launches on the fp32 cores: the order of its arena slots)
            sts = {L.key: ops.new_stats(n, L.cout, dev) for L in chain} if (chain[0].kd == 1 and not pairs) else {}
            for part, group in itertools.groupby(chain, key=lambda L: L.part):
                with self._mm(part):
                    for L in group:
                        # (a route that needs a range table inside the part asks for it here, where the math mode is the part's)
                        route = plan[0][L.key]
                        if plan[1][L.key] != route and self._pair_rng() is not None:
                            route = plan[1][L.key]
                        if route == "pair" and not isinstance(y, ops.PairMap):
                            y, aff = self.to_pairs(y, aff, L.pass_slot), None
                        x, aff_in = y, aff
                        # a branch's last layer writes its slice of an fp32 `cat` itself where there is nothing to apply behind it
                        own = not (L.dst and L.dst[1] == 1 and not L.norm and not isinstance(cat, ops.PairMap))
                        y = torch.empty((*lead(L.edge(size, out=True)), L.cout), dtype=torch.float32, device=dev) if own else \
                            cat[..., L.dst[0]:L.dst[0] + L.cout]
                        aff = self.run_layer(L, route, x, y, aff_in, sts.get(L.key))
                        if L.dst and own:
                            self.join(y, aff, cat, *L.dst)
            last[:] = y, aff

        last = [None, None]
        chains = net.chains()
        branches = [c for c in chains if c[-1].dst]
        ops.fork_join([lambda c=c: run(c) for c in branches], dev) if fork else [run(c) for c in branches]
        run(chains[-1])
        return last

    def run_feature_net(self, imgs, f43=None):
        """imgs [n,3,h,w] in [0,1] -> channels-last features [n,h/4,w/4,128] (reference refiner.py:64-78).
        f43: None = the big calls' kernels (ROUTES) from 4 queries (28 crops) per launch on (below that F(2x2,3x3) is faster); False =
        never (results that are cached per crop must not depend on the batch they were computed in)."""
        pk = self._pack()
        n, _, h, w = imgs.shape
        dev = imgs.device
        big = (n >= F43_MIN_QUERIES * 7) if f43 is None else bool(f43)
        rng = self._pair_rng()
        with self._mm("trunk"):
            taps = trunk_features(pk["vgg"], imgs, ("c3", "c5", "c7_pre"), False, f43=big, rng=rng, pairs=self.pairs_on)   # channels-last

        def tap(f, slot):
            """The L2-normalised tap as its branch reads it: pairs (one pass that normalises and splits), or fp32 in place."""
            def read(pairs):
                if pairs:
                    return ops.l2norm_split16(f[:, 0], 3, rng=(rng, rng.slot(slot)))
                ops.l2norm_rows(f)                  # in place: a tap is never the input of a later layer
                return f
            return read

        maps = {slot: tap(f, slot) for f, slot in zip(taps, ("featnet.f3", "featnet.f5", "featnet.f7"))}
        y, aff = self._run_net(FEATNET, maps, n, (h, w), big, rng is not None, dev, fork=True)
        out = torch.empty((n, 1, h // 4, w // 4, 128), dtype=torch.float32, device=dev)
        ops.affine_act_pool(y, out, aff[0], aff[1], per_n=True)
        return out.view(n, h // 4, w // 4, 128)

    # ------------------------------------------------------------------ 3-D volume net + regressor
    def feature_volumes(self, feats, ref_Ks, ref_poses, K_in, pose_in, h_in, w_in, sn):
        """The two input volumes of the volume net from the crops' features (g6d_refiner_volume_kp): fp32 mean_in [.., sn^3, 2C] and std
        [.., sn^3, C], or — where the embeds run on the pair kernel (a big batch of the fp32 path, ROUTES) — the same as PairMaps
        [qn,sn,sn,sn,2,2C] / [qn,sn,sn,sn,2,C], one exponent slot each."""
        dev = feats.device
        lin = _linspace(sn, dev)
        C = feats.shape[-1]
        args = (feats, ref_Ks.contiguous(), ref_poses.contiguous(), K_in.contiguous(), pose_in.contiguous(), lin, h_in, w_in)
        qn = feats.shape[0] if feats.dim() == 5 else 1
        big = qn >= F43_MIN_QUERIES
        rng = self._pair_rng() if big else None
        if self._plan(VOLUME, qn, (sn,) * 3, big, rng is not None)[0][VOLUME.reader("volume.mean_in").key] == "pair":
            return ops.refiner_volume_kp_pairs(*args, rng_mean=(rng, rng.slot("volume.mean_in")), rng_std=(rng, rng.slot("volume.std")))
        lead = (feats.shape[0],) if feats.dim() == 5 else ()
        mean_in = torch.empty(lead + (sn ** 3, 2 * C), dtype=torch.float32, device=dev)
        std = torch.empty(lead + (sn ** 3, C), dtype=torch.float32, device=dev)
        # projections K @ pose and the volume's rotation are formed inside the kernel (reference refiner.py:208-226)
        return ops.refiner_volume_kp(*args, mean_in, std)

    def run_volume_net(self, mean_in, std, sn):
        """mean_in [sn^3,256], std [sn^3,128] -> code [(sn/8)^3, 512] (reference refiner.py:136-143); or a batch of qn volumes
        ([qn,sn^3,256], [qn,sn^3,128] -> [qn,(sn/8)^3,512]) through the same launches: every InstanceNorm3d keeps one statistics group
        and one affine table per volume.  PairMap volumes (feature_volumes): the layers of the pair kernel read them as they are."""
        pairs_in = isinstance(mean_in, ops.PairMap)
        dev = mean_in.data.device if pairs_in else mean_in.device
        batched = pairs_in or mean_in.dim() == 3
        qn = mean_in.shape[0] if batched else 1
        vol = lambda t: t.view(qn, sn, sn, sn, *t.shape[(-2 if pairs_in else -1):])
        maps = {"volume.mean_in": vol(mean_in), "volume.std": vol(std)}
        code, _ = self._run_net(VOLUME, maps, qn, (sn,) * 3, qn >= F43_MIN_QUERIES, pairs_in, dev, fork=False)
        return code.view(qn, -1, 512) if batched else code.view(-1, 512)

    def run_regressor(self, code):
        """code [v,512] (one query) or [qn,v,512] -> rotation [qn,4] (unit quaternion), offset [qn,2], scale [qn,1]; the 67 MB FC
        weight stream is read once per 8 queries (g6d_linear_gemv_batch)."""
        pk = self._pack()
        qn = code.shape[0] if code.dim() == 3 else 1
        x = ops.linear_gemv(code.reshape(qn, -1), pk["fc0"][0], pk["fc0"][1], act=2)
        x = ops.linear_gemv(x, pk["fc1"][0], pk["fc1"][1], act=2)
        o = ops.linear_gemv(x, pk["heads"][0], pk["heads"][1])
        ops.l2norm_rows(o[:, 0:4])                  # F.normalize(quaternion) in place (rows of four values, row stride 7)
        return o[:, 0:4], o[:, 4:6], o[:, 6:7]

    def _step(self, *a, **k):
        """cfg key 'math_mode' ('bf16' / 'fp16'; default fp32) selects the matrix-core operand precision of this network's conv /
        correlation launches; absent, an enclosing `ops.math_mode(...)` context applies."""
        with ops.math_mode(self.cfg.get("math_mode"), inherit_if_none=True):
            return self._step_fp(*a, **k)

    def _step_fp(self, que_img, K_in, pose_in, ref_imgs, ref_Ks, ref_poses, ref_feats=None):
        """One refinement step.  ref_feats [rfn,fh,fw,C] (single query only): features of the reference crops computed earlier
        (cached_ref_feats) — ref_imgs is then ignored and only the query crop goes through the trunk + feature net.  Single query: que_img [1,3,h,w], K_in [3,3], pose_in [3,4], ref_imgs [rfn,3,h,w], ref_Ks [rfn,3,3],
        ref_poses [rfn,3,4].  Batch of qn <= MAX_BATCH queries (reference forward: refiner.py:249-269 takes [qn,...]): que_img
        [qn,3,h,w], K_in [qn,3,3], pose_in [qn,3,4], ref_imgs [qn,rfn,3,h,w], ref_Ks [qn,rfn,3,3], ref_poses [qn,rfn,3,4] — the
        (rfn+1)*qn crops share the trunk / feature-net launches, the qn volumes the volume-net launches and the FC weight stream."""
        sn = self.cfg["refiner_sample_num"]
        dev = que_img.device
        ops.stats_arena_begin(dev)
        if ref_feats is not None:
            return self._step_from_feats(que_img, K_in, pose_in, ref_feats, ref_Ks, ref_poses)
        batched = ref_imgs.dim() == 5
        qn = ref_imgs.shape[0] if batched else 1
        rfn = ref_imgs.shape[-4]
        h_in, w_in = ref_imgs.shape[-2:]
        if batched:                                    # image order: (refs of query 0, query 0), (refs of query 1, query 1), ...
            imgs = torch.cat([ref_imgs, que_img[:, None]], 1).reshape(qn * (rfn + 1), *ref_imgs.shape[-3:])
        else:
            imgs = torch.cat([ref_imgs, que_img], 0)                                         # query last
        feats = self.run_feature_net(imgs)
        feats = feats.contiguous()
        if batched:
            feats = feats.view(qn, rfn + 1, *feats.shape[1:])
        mean_in, std = self.feature_volumes(feats, ref_Ks, ref_poses, K_in, pose_in, h_in, w_in, sn)
        return self.run_regressor(self.run_volume_net(mean_in, std, sn))

    def _step_from_feats(self, que_img, K_in, pose_in, ref_feats, ref_Ks, ref_poses):
        """The step with the reference crops' features given (cache hits): only the query crop(s) pass the trunk + feature net.
        Single query: ref_feats [rfn,fh,fw,C]; batch: ref_feats [qn,rfn,fh,fw,C] with the [qn,...] operands of _step_fp."""
        sn = self.cfg["refiner_sample_num"]
        dev = que_img.device
        h_in, w_in = que_img.shape[-2:]
        batched = ref_feats.dim() == 5
        qf = self.run_feature_net(que_img)                                               # [qn,fh,fw,C]
        if batched:
            feats = torch.cat([ref_feats, qf[:, None]], 1).contiguous()                  # [qn,rfn+1,fh,fw,C], query last
        else:
            feats = torch.cat([ref_feats, qf], 0).contiguous()
        mean_in, std = self.feature_volumes(feats, ref_Ks, ref_poses, K_in, pose_in, h_in, w_in, sn)
        return self.run_regressor(self.run_volume_net(mean_in, std, sn))

    def forward(self, data):
        """Same dict contract as the reference (refiner.py:249-269)."""
        is_inference = data["inference"] if "inference" in data else False
        que, ref = data["que_imgs_info"], data["ref_imgs_info"]
        qn_all = que["imgs"].shape[0]
        if qn_all == 1:
            outs = [self._step(que["imgs"], que["Ks_in"][0], que["poses_in"][0], ref["imgs"][0], ref["Ks"][0], ref["poses"][0])]
        else:                                                                  # the queries of a chunk share every launch
            outs = [self._step(que["imgs"][q0:q0 + MAX_BATCH], que["Ks_in"][q0:q0 + MAX_BATCH], que["poses_in"][q0:q0 + MAX_BATCH],
                               ref["imgs"][q0:q0 + MAX_BATCH], ref["Ks"][q0:q0 + MAX_BATCH], ref["poses"][q0:q0 + MAX_BATCH])
                    for q0 in range(0, qn_all, MAX_BATCH)]
        out = {"rotation": ops.cat1([o[0] for o in outs], 0), "offset": ops.cat1([o[1] for o in outs], 0),
               "scale": ops.cat1([o[2] for o in outs], 0)}
        if not is_inference:
            sn = self.cfg["refiner_sample_num"]
            g = torch.linspace(-1, 1, sn, dtype=torch.float32, device=que["imgs"].device)
            V = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, sn ** 3, 3) @ que["poses_in"][:, :3, :3]
            out["grids"] = pose_apply_th(que["poses_in"], V)
        return out

    # ------------------------------------------------------------------ estimator API
    def load_ref_imgs(self, ref_database, ref_ids):
        """reference refiner.py:270-272.  A new database drops whatever an own image cache held for the previous one
        (Gen6DEstimator.build shares and clears its cache itself)."""
        cache = getattr(self, "image_cache", None)
        if ref_database is not self.ref_database and cache is not None and not cache.holds(ref_database):
            cache.clear()
        if ref_database is not self.ref_database:
            self.feat_cache.clear()
        self.ref_database = ref_database
        self.ref_ids = ref_ids

    def refine_que_imgs(self, que_img, que_K, in_pose, size=128, ref_num=6, ref_even=False):
        """One refinement step with the reference's signature (refiner.py:275-341): que_img uint8 [H,W,3] (numpy or a
        device tensor), que_K [3,3], in_pose [3,4] -> refined pose [3,4] float32.  The look-at crop of the query and the
        6 aligned reference crops are device warps (g6d_warp_perspective) of images cached on the GPU; the pose algebra
        stays on the host."""
        from .. import estimator as E
        from .. import geometry as G
        margin, even_num = 0.05, min(128, len(self.ref_ids))
        dev = self.device_()
        cache = getattr(self, "image_cache", None)
        if cache is None:
            cache = self.image_cache = E.DeviceImageCache(dev)
        db = E.NormalizedDatabase(self.ref_database)
        in_pose = G.normalize_pose(np.asarray(in_pose, np.float64), db.scale, db.offset)
        center, diameter = db.object_center, db.object_diameter
        que_K = np.asarray(que_K, np.float64)
        _, new_f = G.let_me_look_at(in_pose, que_K, center)
        in_dist = np.linalg.norm(G.pose_inverse(in_pose)[:, 3] - center)
        scale = size * (1 - margin) / diameter * in_dist / new_f
        position = G.project_points(center[None], in_pose, que_K)[0][0]
        K_warp, pose_warp, pose_rect, H = G.look_at_crop_params(que_K, in_pose, position, 0, scale, size, size)
        if not torch.is_tensor(que_img):
            que_img = torch.from_numpy(np.ascontiguousarray(que_img)).to(dev)
        que_warp = ops.warp_perspective(que_img, H, size, size)
        ref_ids = E.select_reference_img_ids_refinement(db, center, self.ref_ids, pose_warp, ref_num, ref_even, even_num, cache)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        que_t = que_warp.float().div_(255).permute(2, 0, 1)[None].contiguous()
        step = self.angle_step()
        with torch.no_grad():
            out = self.range_guarded(lambda: self._refine_step(step, db, ref_ids, size, margin, pose_warp, K_warp, cache, que_t, f))
        quat, offset, scale_pr = out[:4], out[4:6], 2 ** out[6]
        pose_sim = G.compose_sim_pose(scale_pr, quat, offset, pose_warp, center)
        pose_pr = G.pose_sim_to_pose_rigid(pose_sim, pose_warp, K_warp, K_warp, center)
        pose_pr = G.pose_compose(pose_pr, G.pose_inverse(pose_rect))
        return G.denormalize_pose(pose_pr, db.scale, db.offset)

    def _range_fallback(self):
        # reference-crop features cached from pair maps that left the window are not reused
        self.feat_cache.clear()

    def _refine_step(self, step, db, ref_ids, size, margin, pose_warp, K_warp, cache, que_t, f):
        from .. import estimator as E
        if step > 0:
            # alignment angles snapped to the grid: the crop of a view depends on (view, bucket) only -> cached features
            ref_Ks, ref_poses, Hs, buckets = E.reference_view_params(db, ref_ids, size, margin, True, pose_warp, K_warp, angle_step=step)
            keys = [(id(self.ref_database), str(i), int(b), int(size)) for i, b in zip(ref_ids, buckets)]
            make = lambda miss: torch.stack([ops.warp_perspective(cache.get(db, ref_ids[k]), Hs[k], size, size) for k in miss], 0) \
                .float().div_(255).permute(0, 3, 1, 2).contiguous()
            ref_feats = self.cached_ref_feats(keys, make)
            rot, off, scl = self._step(que_t, f(K_warp), f(pose_warp), None, f(ref_Ks), f(ref_poses), ref_feats=ref_feats)
        else:
            ref_imgs, _, ref_Ks, ref_poses, _ = E.normalize_reference_views(db, ref_ids, size, margin, cache, True, pose_warp, K_warp,
                                                                         with_masks=False)
            rot, off, scl = self._step(que_t, f(K_warp), f(pose_warp), ref_imgs.float().div_(255).permute(0, 3, 1, 2).contiguous(),
                                       f(ref_Ks), f(ref_poses))
        return torch.cat([rot[0], off[0], scl[0]]).cpu().numpy()

    def refine_step_tensors(self, que_img_u8, K_in, pose_in, ref_imgs_u8, ref_Ks, ref_poses):
        """Numpy boundary of one step after the host-side warps: uint8 crops [h,w,3] / [rfn,h,w,3], float32 K/poses
        -> (quat [4], scale (=2**s) [1], offset [2]) numpy, as consumed at reference refiner.py:327-331."""
        dev = self.device_()
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        q = torch.from_numpy(np.ascontiguousarray(que_img_u8)).to(dev).float().div_(255).permute(2, 0, 1)[None].contiguous()
        r = torch.from_numpy(np.ascontiguousarray(ref_imgs_u8)).to(dev).float().div_(255).permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            rot, off, scl = self._step(q, f(K_in), f(pose_in), r, f(ref_Ks), f(ref_poses))
        return rot[0].cpu().numpy(), 2 ** scl[0].cpu().numpy(), off[0].cpu().numpy()
