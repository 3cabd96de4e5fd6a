"""Detector — drop-in for the reference's network/detector.py:Detector (same constructor, state_dict keys, methods and
output dicts), driving hand-written HIP kernels end to end.

For the 4 detection scales of a batch of queries at once (reference detect_impl, detector.py:232-266):
    own trunk                       one launch per layer over the whole pyramid (backbone.trunk_route: fp16 hi / lo pairs on the direct
                                    kernel, or F(4x4,3x3) on fp32 MFMA) -> x0 @1/8, x1 @1/16, x2 @1/32
    correlation x3                  query features correlated with the reference feature maps used as filters
                                    (F.conv2d(que_x, ref_x, padding=7/3/1), detector.py:222-224), on the kernel Detector.corr_routes names:
                                    at 32 references the 15x15 and 7x7 levels on g6d_corr16_multi (the trunk hands them over in its
                                    pair format), otherwise as blocks of 3x3 in the F(4x4,3x3) domain (g6d_corr2d_wino43_multi; the 7x7
                                    filters zero-extended to 9x9); the 3x3 level on g6d_corr2d_patch_multi; calls of at least
                                    CORR_FFT_MIN_QUERIES queries run the 15x15 level in the frequency domain on the fp32 tap
                                    (route "fft": ops.corr_fft_multi, csrc/corr_fft.hip)
    g6d_detector_assemble           nearest up-sampling, (x-mu)/sigma, clip, bilinear resize to (h/8,w/8), stack
then g6d_detector_score_mlp_max     score_conv MLP + max over references, never materialising [64,rfn,hs,ws]
     g6d_conv_igemm x7              the three 3x3 heads (first layers merged into one 64->192 conv)
     g6d_detector_decode            arg-max + offset/scale gather.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops, parallel, specs
from .backbone import (is_16bit, pack_trunk, trunk_features, trunk_features_multi, trunk_route, winograd43_corr_filters,
                       winograd43_corr_filters_padded)
from .params import ParamBank, fold_vgg

_TAPS = ("c5", "c7_pre", "p7")   # the trunk taps of the three correlation levels (15x15, 7x7, 3x3 filters at 120 x 120 references)
MAX_BATCH = 16       # most queries that share one set of launches; _detect_impl_fp cuts the chunk further for larger images (the pyramid's
                     # first layers address all scales of the batch with 32-bit offsets from one base, < 2^29 floats: 16 images of
                     # 480x640 at 64 channels; 32 would not fit)
CORR_FFT_MIN_QUERIES = 4     # queries per call from which the 15x15 level runs in the frequency domain (ops.corr_fft_multi).  Its three
                             # launches beat the one corr16 launch by more than that launch's own spread at every batch measured, 1 included
                             # (profiles/r29_corr_fft.md); the floor of 4 keeps the tracker's two-query acquisition chunks and single
                             # queries on the launches they have


class Detector(ParamBank):
    default_cfg = {
        "vgg_score_stats": [[36.264317, 13.151907], [13910.291, 5345.965], [829.70807, 387.98788]],
        "vgg_score_max": 10,
        "detection_scales": [-1.0, -0.5, 0.0, 0.5],
        "train_feats": False,
    }

    def __init__(self, cfg):
        self.cfg = {**self.default_cfg, **cfg}
        super().__init__(specs.detector_rows())
        if len(self.cfg["detection_scales"]) != 4:
            raise NotImplementedError("score_conv expects 3 levels x 4 detection scales (12 channels)")
        self.pool_ratio = 8
        self.ref_center_feats = None     # three [rfn, k*k, 512] correlation filters
        self.ref_wino15_43 = None        # the 15x15 level's filters for the F(4x4,3x3) kernel (winograd43_corr_filters), rfn % 32 == 0
        self.ref_wino7_43 = None         # the 7x7 level's filters, zero-extended to 9x9, for the F(4x4,3x3) kernel
        self._corr16 = {}                # (level, mode) -> the level's filters for g6d_corr16_multi, built on first use
        self._corr_fft = None            # the 15x15 level's filter spectra for ops.corr_fft_multi, built on first use
        self.ref_shape = None
        self.rank, self.world, self.group = 0, 1, None
        self.sharded = False

    def set_shard(self, rank, world, group=None, force_collectives=False):
        """Reference-sharded mode: this rank correlates the query against references
        parallel.shard_range(rfn, rank, world) only; correlation, score assembly and the score MLP are per-reference, and
        `torch.max(scores, 2)` over the references (detector.py:247) becomes one all-reduce(MAX) of the [hs*ws, 64]
        feature map (1.2 MB at 60x80) over torch.distributed (RCCL).  The query trunk and the heads are replicated.
        `force_collectives`: issue the all-reduce at world size 1 as well (see ViewpointSelector.set_shard)."""
        self.rank, self.world, self.group = int(rank), int(world), group
        self.sharded = self.world > 1 or bool(force_collectives)

    # ------------------------------------------------------------------ weights
    def _pack(self):
        if self._packed is None:
            pk = {"vgg": pack_trunk(fold_vgg(self, "backbone.features"))}
            w0, b0 = self.conv_w("score_conv.0")
            w1, b1 = self.conv_w("score_conv.2")
            pk["mlp"] = (w0.reshape(64, 12).contiguous(), b0, w1.reshape(64, 64).contiguous(), b1)
            heads = ("score_predict", "scale_predict", "offset_predict")
            l0 = [self.conv_w(f"{h}.0") for h in heads]
            pk["h0"] = (torch.cat([w for w, _ in l0], 0).contiguous(), torch.cat([b for _, b in l0], 0).contiguous())
            pk["h1"] = [self.conv_w(f"{h}.2") for h in heads]
            # the three heads' last convs (1 + 1 + 2 output channels on their own 64-channel inputs) as ONE conv 192 -> 4 with
            # block-diagonal weights: the zero blocks add exact zeros, one launch instead of three latency-bound ones
            l2 = [self.conv_w(f"{h}.4") for h in heads]
            w4 = torch.zeros((sum(w.shape[0] for w, _ in l2), 9, 192), dtype=torch.float32, device=l2[0][0].device)
            row = 0
            for i, (w, _) in enumerate(l2):
                w4[row:row + w.shape[0], :, 64 * i:64 * i + 64] = w
                row += w.shape[0]
            pk["h2"] = (w4.contiguous(), torch.cat([b for _, b in l2], 0).contiguous())
            self._packed = pk
        return self._packed

    # ------------------------------------------------------------------ trunk
    def extract_feats(self, imgs):
        """imgs [n,3,h,w] in [0,1] -> channels-last x0,x1,x2: [n,1,h/8,w/8,512], [.. /16 ..], [.. /32 ..]."""
        return trunk_features(self._pack()["vgg"], imgs, _TAPS, False)

    def load_impl(self, ref_imgs):
        """ref_imgs [rfn,3,h,w] in [0,1]; nearest resize to 120x120, trunk, keep as correlation filters
        (reference detector.py:199-205)."""
        b, e = parallel.shard_range(ref_imgs.shape[0], self.rank, self.world)
        if e == b:
            raise ValueError("more ranks than reference views")
        ref_imgs = F.interpolate(ref_imgs[b:e], size=(120, 120))
        feats = self.extract_feats(ref_imgs)                       # [rfn_local,1,k,k,512]
        self.ref_center_feats = [f.reshape(f.shape[0], f.shape[2] * f.shape[3], 512).contiguous() for f in feats]
        self.ref_ksize = [f.shape[2] for f in feats]               # 15, 7, 3
        self._corr16 = {}
        self._corr_fft = None
        self.ref_shape = [120, 120]
        # F(4x4,3x3)-domain filters of the 15x15 and 7x7 levels for the "wino43" route (the reference views used as filters: transformed
        # once per object; whether a call takes the route depends on its math mode and pair setting, so they exist whenever it can)
        wino43 = self.ref_center_feats[0].shape[0] % 32 == 0
        self.ref_wino15_43 = winograd43_corr_filters(self.ref_center_feats[0], 15) if wino43 else None
        self.ref_wino7_43 = winograd43_corr_filters_padded(self.ref_center_feats[1], 7)[0] if wino43 else None

    def _corr16_filters(self, level, mode):
        """The reference-centre features of a level packed for g6d_corr16_multi (ops.corr16_pack), built on first use per (level, mode)."""
        if (level, mode) not in self._corr16:
            self._corr16[level, mode] = ops.corr16_pack(self.ref_center_feats[level], mode)
        return self._corr16[level, mode]

    def _corr_fft_filters(self):
        """The 15x15 level's filter spectra (ops.corr_fft_spectra), built on first use: reference state, the same for every query."""
        if self._corr_fft is None:
            self._corr_fft = ops.corr_fft_spectra(self.ref_center_feats[0])
        return self._corr_fft

    def corr_routes(self, hq, wq, qn=1):
        """The kernel that correlates each level (15x15, 7x7, 3x3 filters) with the references for [qn,3,hq,wq] queries in the current math
        mode and pair setting:
          "fft"     ops.corr_fft_multi, the 15x15 level in the frequency domain (32 x 32 windows, fp32): where "corr16" would be taken on
                    the fp32 path (pairs on, 32 references, not sharded) for calls of at least CORR_FFT_MIN_QUERIES queries; the trunk hands
                    the level over as its fp32 tap.  cfg key 'corr_fft': None = that rule, False = never, True = at any batch (tools, tests)
          "corr16"  g6d_corr16_multi: the pyramid trunk runs on the direct kernel and hands the level over in its 16-bit / pair format
                    (32 references)
          "wino43"  blocks of 3x3 in the F(4x4,3x3) domain (fp32, rfn % 32 == 0: 20.25 instead of 49 multiplications per output at 7x7)
          "patch"   g6d_corr2d_patch_multi, one launch over all scales (rfn <= 32)
          "conv"    the generic conv, one launch per scale."""
        sizes = [self._scale_size(hq, wq, sc) for sc in self.cfg["detection_scales"]]
        trunk16 = trunk_route(self._pack()["vgg"], sizes, _TAPS, f43=True, pairs=self.pairs_on) == "direct"
        rfn = self.ref_center_feats[0].shape[0]
        routes = []
        for k in self.ref_ksize:
            if k in (15, 7) and trunk16 and rfn == 32:
                want = self.cfg.get("corr_fft")
                fft = k == 15 and not ops.MATH_MODE and not self.sharded and want is not False and (want or qn >= CORR_FFT_MIN_QUERIES)
                routes.append("fft" if fft else "corr16")
            elif k in (15, 7) and rfn % 32 == 0 and not ops.MATH_MODE:
                routes.append("wino43")
            else:
                routes.append("patch" if rfn <= 32 else "conv")
        return routes

    # ------------------------------------------------------------------ detection
    def _scores_one_scale(self, que_img, scale_idx, stacked, hs, ws):
        self._scores_from_feats(self.extract_feats(que_img), scale_idx, stacked, hs, ws)

    def _scores_from_pyramid(self, feats, routes, scale_ids, stacked, hs, ws):
        """All scales (and all queries of the batch) at once: every correlation level is ONE launch over the maps of all scales on
        the kernel routes[l] names (corr_routes; the tiles of all maps form one work list: fewer splits, the small maps fill the chip the
        large one leaves over); the assembly is one launch per scale.  feats[i][l]: [qn,1,h,w,512], or the trunk's 16-bit / pair format
        on the "corr16" route."""
        rfn = self.ref_center_feats[0].shape[0]
        dev = stacked.device
        qn = feats[0][0].shape[0]
        maps = [[None] * 3 for _ in feats]
        for l, (wref, k, route) in enumerate(zip(self.ref_center_feats, self.ref_ksize, routes)):
            xs = [f[l] for f in feats]
            assert is_16bit(xs[0]) == (route == "corr16"), "the trunk did not hand the level over in the format of its route"
            if route == "corr16":
                # 16-bit activations (reduced precision) or fp16 hi / lo pairs (fp32 path): the halo-patch correlation kernel on the 16-bit
                # matrix cores (csrc/corr16.hip, corr16_kernel)
                mode = 3 if len(xs[0].shape) == 5 else (1 if xs[0].dtype == torch.bfloat16 else 2)
                filt = self._corr16_filters(l, mode)
                outs = [torch.empty((qn, 1, x.shape[1], x.shape[2], rfn), dtype=torch.float32, device=dev) for x in xs]
                ops.corr16_multi(xs, filt, outs)
                for i, o in enumerate(outs):
                    maps[i][l] = o.reshape(qn * o.shape[2] * o.shape[3], rfn)
                continue
            if route == "fft":
                # the fp32 tap through forward FFT, per-bin products on the fp32 matrix cores and inverse FFT (csrc/corr_fft.hip)
                outs = [torch.empty((qn, 1, x.shape[2], x.shape[3], rfn), dtype=torch.float32, device=dev) for x in xs]
                ops.corr_fft_multi([x.contiguous() for x in xs], self._corr_fft_filters(), outs)
                for i, o in enumerate(outs):
                    maps[i][l] = o.reshape(qn * o.shape[2] * o.shape[3], rfn)
                continue
            # one launch over all scales addresses the maps with 32-bit offsets from a common base (offset + extent < 2^29 floats on the
            # Winograd routes): maps that do not come out of one buffer (a trunk that allocates every scale on its own) are gathered first
            lo = min(x.data_ptr() for x in xs)
            hi = max(x.data_ptr() + x.numel() * 4 for x in xs)
            if hi - lo >= (1 << 31) or not all(x.is_contiguous() for x in xs):
                seg = ops.alloc_like_segments([tuple(x.shape) for x in xs], dev)
                for d_, x in zip(seg, xs):
                    d_.copy_(x)
                xs = seg
            if route == "conv":
                outs = [torch.empty((qn, 1, x.shape[2], x.shape[3], rfn), dtype=torch.float32, device=dev) for x in xs]
                for x, o in zip(xs, outs):
                    ops.conv(x, wref, None, o, ksize=(1, k, k), pad=(0, k // 2, k // 2))
            else:
                outs = ops.alloc_like_segments([(qn, 1, x.shape[2], x.shape[3], rfn) for x in xs], dev)
                if route == "patch":
                    ops.corr2d_patch_multi(xs, wref, outs, k)
                elif k == 15:
                    ops.corr2d_wino43_multi([x.contiguous() for x in xs], self.ref_wino15_43, outs, 5)
                else:
                    ops.corr2d_wino43_multi([x.contiguous() for x in xs], self.ref_wino7_43, outs, 3, k_true=7)
            for i, o in enumerate(outs):
                maps[i][l] = o.reshape(qn * o.shape[2] * o.shape[3], rfn)
        for f, si, m in zip(feats, scale_ids, maps):
            hc, wc = (f[0].shape[1], f[0].shape[2]) if is_16bit(f[0]) else (f[0].shape[2], f[0].shape[3])
            ops.detector_assemble(m[0], m[1], m[2], hc, wc, self.cfg["vgg_score_stats"],
                                  float(self.cfg["vgg_score_max"]), hs, ws, si, stacked, batch=qn)

    def _scores_from_feats(self, feats, scale_idx, stacked, hs, ws):
        x0, x1, x2 = feats
        rfn = self.ref_center_feats[0].shape[0]
        qn = x0.shape[0]
        maps = []
        for x, wref, k in zip((x0, x1, x2), self.ref_center_feats, self.ref_ksize):
            _, _, h, w, _ = x.shape
            o = torch.empty((qn, 1, h, w, rfn), dtype=torch.float32, device=x.device)
            if k >= 7 and rfn <= 32 and qn == 1:       # 15x15 and 7x7 levels: input patch kept in LDS and walked by the kx taps
                ops.corr2d_patch(x, wref, o, k)
            else:
                ops.conv(x, wref, None, o, ksize=(1, k, k), pad=(0, k // 2, k // 2))
            maps.append(o.reshape(qn * h * w, rfn))
        hc, wc = x0.shape[2], x0.shape[3]
        ops.detector_assemble(maps[0], maps[1], maps[2], hc, wc, self.cfg["vgg_score_stats"],
                              float(self.cfg["vgg_score_max"]), hs, ws, scale_idx, stacked, batch=qn)

    @staticmethod
    def _scale_size(hq, wq, scale):
        """Size of the query at a detection scale: round(h * 2^s), rounded UP to a multiple of 32 (reference detector.py:237-239)."""
        ht, wt = int(np.round(hq * 2 ** scale)), int(np.round(wq * 2 ** scale))
        if ht % 32 != 0: ht = (ht // 32 + 1) * 32
        if wt % 32 != 0: wt = (wt // 32 + 1) * 32
        return ht, wt

    def _detect_batch(self, que_imgs, multi=True):
        """que_imgs [qn,3,hq,wq]: the whole batch goes through every launch together (trunk pyramid segments of qn images,
        correlation tiles of qn maps per scale, heads with M = qn*hs*ws) — reference API: detector.py:291-304 takes [qn,H,W,3]."""
        pk = self._pack()
        qn, _, hq, wq = que_imgs.shape
        hs, ws = hq // 8, wq // 8
        dev = que_imgs.device
        rfn = self.ref_center_feats[0].shape[0]
        P = hs * ws
        stacked = torch.empty((qn * P, rfn, 12), dtype=torch.float32, device=dev)
        def resized(scale):
            return F.interpolate(que_imgs, size=self._scale_size(hq, wq, scale), mode="bilinear")

        # the scales are independent until `stacked` is complete: largest first on the main stream
        order = sorted(enumerate(self.cfg["detection_scales"]), key=lambda t: -t[1])
        if multi:
            # every trunk layer is ONE launch over the whole pyramid (the small scales fill the blocks the large ones leave
            # over); the correlations of the scales then run side by side
            # the image pyramid in ONE launch (g6d_resize_bilinear_pyramid; the scale of the query's own size is the query itself)
            pyr = ops.resize_bilinear_pyramid(que_imgs, [self._scale_size(hq, wq, sc) for _, sc in order])
            routes = self.corr_routes(hq, wq, qn)
            t16 = tuple(tap for tap, r in zip(_TAPS, routes) if r == "corr16")     # taps handed over in the trunk's 16-bit / pair format
            feats = trunk_features_multi(pk["vgg"], pyr, _TAPS, f43=True, taps16=t16, rng=self._pair_rng(), pairs=self.pairs_on)
            self._scores_from_pyramid(feats, routes, [si for si, _ in order], stacked, hs, ws)
        else:
            ops.fork_join([(lambda si=si, sc=sc: self._scores_one_scale(resized(sc), si, stacked, hs, ws)) for si, sc in order], dev)
        feats = ops.detector_score_mlp_max(stacked, *pk["mlp"])               # [qn*P,64], max over the local references
        if self.sharded:
            parallel.all_reduce_(feats, "max", self.group)
        k3, p3 = (1, 3, 3), (0, 1, 1)
        a = torch.empty((qn, 1, hs, ws, 192), dtype=torch.float32, device=dev)
        ops.conv(feats.view(qn, 1, hs, ws, 64), pk["h0"][0], pk["h0"][1], a, ksize=k3, pad=p3, out_act=1)
        b = torch.empty_like(a)
        o4 = torch.empty((qn, 1, hs, ws, 4), dtype=torch.float32, device=dev)
        for i in range(3):
            w1, b1 = pk["h1"][i]
            ops.conv(a[..., 64 * i:64 * i + 64], w1, b1, b[..., 64 * i:64 * i + 64], ksize=k3, pad=p3, out_act=1)
        ops.conv(b, pk["h2"][0], pk["h2"][1], o4, ksize=k3, pad=p3)            # score | scale | offset x, y
        o4 = o4.view(qn * P, 4)                                                # score, scale, offset x, offset y
        res = ops.detector_decode(o4[:, 0:1], o4[:, 2:4], o4[:, 1:2], hs, ws, self.pool_ratio, batch=qn)
        return o4.view(qn, hs, ws, 4), res.view(qn, 5), (hs, ws)

    def detect_impl(self, *a, **k):
        """cfg key 'math_mode' ('bf16' / 'fp16'; default fp32) selects the matrix-core operand precision of this network's conv /
        correlation launches; absent, an enclosing `ops.math_mode(...)` context applies."""
        with ops.math_mode(self.cfg.get("math_mode"), inherit_if_none=True):
            return self._detect_impl_fp(*a, **k)

    def _detect_impl_fp(self, que_imgs):
        """que_imgs [qn,3,hq,wq] in [0,1] -> the reference's output dict (detector.py:232-266) plus
        'positions' [qn,2] and 'scales' [qn] already decoded on the device."""
        outs, results = [], []
        # the queries of a chunk share every launch; the chunk is sized by the image: the one-launch-per-layer pyramid addresses all
        # scales of the batch with 32-bit offsets from one base (< 2^29 floats; the widest tensor is the first layer's pooled output,
        # 64 channels at a quarter of the pixels) — 16 queries of 480x640, 9 of 720x1280; an image whose pyramid alone exceeds the
        # reach runs one trunk pass per scale
        _, _, hq, wq = que_imgs.shape
        per_query = sum(self._scale_size(hq, wq, sc)[0] * self._scale_size(hq, wq, sc)[1] for sc in self.cfg["detection_scales"]) // 4 * 64
        step = max(1, min(MAX_BATCH, ((1 << 29) - 1) // per_query))
        multi = per_query < (1 << 29)
        for q0 in range(0, que_imgs.shape[0], step):
            o4, res, _ = self._detect_batch(que_imgs[q0:q0 + step].contiguous(), multi)
            outs.append(o4.permute(0, 3, 1, 2))
            results.append(res)
        o = ops.cat1(outs, 0)                                                  # qn,4,hs,ws
        r = ops.cat1(results, 0)
        return {"scores": o[:, 0:1], "select_pr_scale": o[:, 1:2], "select_pr_offset": o[:, 2:4],
                "que_select_id": r[:, 3:5].round().long(), "pool_ratio": self.pool_ratio,
                "positions": r[:, 0:2], "scales": r[:, 2]}

    def forward(self, data):
        self.load_impl(data["ref_imgs_info"]["imgs"])
        return self.detect_impl(data["que_imgs_info"]["imgs"])

    @staticmethod
    def parse_detection(scores, scales, offsets, pool_ratio):
        """Same contract as BaseDetector.parse_detection (detector.py:97-121), torch ops on the caller's device."""
        qn, _, hs, ws = scores.shape
        flat = torch.argmax(scores.flatten(1), 1)
        sy, sx = flat // ws, flat % ws
        ar = torch.arange(qn, device=scores.device)
        pos = (torch.stack([sx, sy], -1) + offsets[ar, :, sy, sx] + 0.5) * pool_ratio - 0.5
        return pos, 2 ** scales[ar, 0, sy, sx]

    # ------------------------------------------------------------------ numpy API used by Gen6DEstimator
    def load_ref_imgs(self, ref_imgs):
        """ref_imgs: uint8 [rfn,h,w,3] (reference detector.py:277-289)."""
        x = torch.from_numpy(np.ascontiguousarray(ref_imgs)).to(self.device_()).float().div_(255).permute(0, 3, 1, 2)
        with torch.no_grad():
            self.range_guarded(lambda: self.load_impl(x.contiguous()))

    def detect_que_imgs(self, que_imgs):
        """que_imgs: uint8 [qn,h,w,3] -> {'positions': [qn,2], 'scales': [qn]} numpy (reference detector.py:291-304)."""
        x = torch.from_numpy(np.ascontiguousarray(que_imgs)).to(self.device_()).float().div_(255).permute(0, 3, 1, 2)
        with torch.no_grad():
            out = self.range_guarded(lambda: self.detect_impl(x.contiguous()))
        return {"positions": out["positions"].cpu().numpy(), "scales": out["scales"].cpu().numpy()}
