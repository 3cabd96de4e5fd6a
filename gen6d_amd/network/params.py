"""ParamBank: an nn.Module whose state_dict() has exactly the reference's keys and shapes (gen6d_amd/specs.py), so
`load_state_dict(torch.load('data/model/<name>/model_best.pth')['network_state_dict'])` works unchanged
(reference estimator.py:117-125), plus helpers that repack weights into the layouts the HIP kernels consume."""
import torch
import torch.nn as nn

from .. import ops, specs


class ConvW(tuple):
    """(weight [Cout,taps,Cin], bias) as the conv kernels take them, plus `.u`: the same filters transformed for the Winograd
    kernel (None when the layer never qualifies), `.u43`: the same for the F(4x4,3x3) kernel (G6dConv.weight_wino43; only for the
    layers that ask for it), and `.w16(mode)`: the filters of the direct 16-bit kernel.  Unpacks like the plain pair."""

    def __new__(cls, w, b, u=None, u43=None):
        t = super().__new__(cls, (w, b))
        t.u, t.u43, t._w16 = u, u43, {}
        return t

    def w16(self, mode, layout=1):
        """The filters for the direct kernel on 16-bit activations (ops.conv16_pack, fragment-major) in `mode` (1 / 2 = rounded to bf16 /
        fp16, 3 = fp16 hi / lo pairs), built on first use.  layout 2: a 3x3x3 layer's depth taps folded into the reduction."""
        key = mode if layout == 1 else (mode, layout)
        if key not in self._w16:
            self._w16[key] = ops.conv16_pack(self[0], mode, layout=layout)
        return self._w16[key]


class ParamBank(nn.Module):
    def __init__(self, rows):
        super().__init__()
        self._roles = {}
        for key, shape, role in specs.expand(rows):
            *path, leaf = key.split(".")
            mod = self
            for name in path:
                if name not in mod._modules:
                    mod.add_module(name, nn.Module())
                mod = mod._modules[name]
            if role in ("weight", "bias", "gamma", "beta"):
                init = torch.ones(shape) if role == "gamma" else torch.zeros(shape)
                mod.register_parameter(leaf, nn.Parameter(init, requires_grad=False))
            elif role == "count":
                mod.register_buffer(leaf, torch.zeros((), dtype=torch.long))
            else:
                mod.register_buffer(leaf, torch.ones(shape) if role == "rvar" else torch.zeros(shape))
            self._roles[key] = role
        self._packed = None

    # any weight change invalidates the packed copies (the packed trunks / heads with their transformed and 16-bit filters) and the pair
    # maps' exponents and record (the range table is reset in place, not dropped: captured graphs hold pointers into it)
    sharded = False                      # reference-sharded mode (Detector / ViewpointSelector.set_shard)

    def _reset_derived(self):
        self._packed = None
        self.__dict__.pop("_range_seen", None)
        t = self.__dict__.get("_range")
        if t is not None:
            t.reset()

    def load_state_dict(self, *a, **k):
        self._reset_derived()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._reset_derived()
        return super()._apply(fn, *a, **k)

    # ---- range control of the fp32 path's fp16 hi / lo pair maps (ops.RangeTable, ops.pair_exponent) -------------------------------------
    @property
    def pairs_on(self):
        """Whether the fp32 path may store activations as fp16 hi / lo pairs (products on the 16-bit matrix cores): not with the cfg key
        'fp32_cores' (read at call time, like 'math_mode') and not while a call is recomputed on the fp32-core routes."""
        return not (self.cfg.get("fp32_cores") or self.__dict__.get("_pairs_off", False))

    @property
    def range_fallbacks(self):
        """Calls recomputed on the fp32-core routes because a pair map left the window."""
        return self.__dict__.get("_range_fallbacks", 0)

    def range_table(self):
        """The network's exponent table and range record (one slot per pair-producing call site), created on first use."""
        t = self.__dict__.get("_range")
        if t is None or t.device != self.device_():
            t = self._range = ops.RangeTable(self.device_())
        return t

    def _pair_rng(self):
        """The range table for this network's pair maps: None while its pair routes are off, in a reduced-precision mode or off the GPU."""
        return self.range_table() if (self.pairs_on and not ops.MATH_MODE and self.device_().type == "cuda") else None

    def range_check(self):
        """Read and clear the record (synchronises).  If a map left the window since the last check: raise in the reference-sharded mode
        (a per-rank recompute would desynchronise the collectives), else update the exponents of the slots that left it, count a fallback
        and return True (the caller recomputes on the fp32-core routes)."""
        t = self.__dict__.get("_range")
        if t is None or not t.names:
            return False
        a = t.read()
        t.clear()
        self._range_seen = {n: max(v, self.__dict__.get("_range_seen", {}).get(n, 0.0)) if v == v else v for n, v in a.items()}
        bad = {n: v for n, v in a.items() if ops.pair_out_of_window(v, t.e[t.names[n]])}
        if not bad:
            return False
        if self.sharded:
            raise RuntimeError(f"{type(self).__name__}: fp16 pair maps left the representable window in the reference-sharded mode "
                               f"({', '.join(f'{n}: max |v| = {v:g}' for n, v in bad.items())}); a per-rank fp32 recompute would desynchronise "
                               "the collectives")
        t.set_exponents({n: ops.pair_exponent(v, t.e[t.names[n]]) for n, v in bad.items()})
        self._range_fallbacks = self.range_fallbacks + 1
        return True

    def range_guarded(self, fn):
        """fn() (one call of this network that ends in a synchronisation anyway), checked: recomputed once on the fp32-core routes when a
        pair map left the window.  Non-finite values the fp32 routes produce as well are returned as they are."""
        return range_guarded((self,), fn)

    def _range_fallback(self):
        """Hook: drop state derived from a call whose pair maps left the window (before its recompute)."""

    def range_report(self):
        """{slot name: {"A": largest |v| recorded since the weights were loaded, "e": current exponent}}."""
        t = self.__dict__.get("_range")
        if t is None:
            return {}
        seen = self.__dict__.get("_range_seen", {})
        return {n: {"A": seen.get(n, 0.0), "e": t.e[i]} for n, i in t.names.items()}

    def p(self, key):
        *path, leaf = key.split(".")
        mod = self
        for name in path:
            mod = mod._modules[name]
        t = mod._parameters.get(leaf)
        return (t if t is not None else mod._buffers[leaf]).detach()

    def device_(self):
        return next(self.parameters()).device

    def conv_w(self, prefix, cin_pad=None, wino_kd=0, f43=False):
        """[Cout,Cin,*k] -> ConvW([Cout,taps,Cin] contiguous (Cin zero-padded to cin_pad), bias).  wino_kd = 1 / 3: the layer is
        a stride-1 (1,3,3) / (3,3,3) convolution — also keep its Winograd-domain filters (`.u`, see G6dConv.weight_wino); f43: and those of
        the F(4x4,3x3) kernel (`.u43`, Cout % 64 == 0)."""
        w = self.p(prefix + ".weight")
        co, ci = w.shape[:2]
        w = w.reshape(co, ci, -1).permute(0, 2, 1)
        if cin_pad is not None and cin_pad != ci:
            w = torch.nn.functional.pad(w, (0, cin_pad - ci))
        w = w.contiguous()
        u = u43 = None
        if wino_kd and ci % 8 == 0 and co % 32 == 0 and w.shape[1] == 9 * wino_kd:
            from .backbone import winograd_filters_taps, winograd43_filters_taps
            u = winograd_filters_taps(w, wino_kd)
            if f43 and co % 64 == 0:
                u43 = winograd43_filters_taps(w, wino_kd)
        return ConvW(w, self.p(prefix + ".bias").contiguous(), u, u43)


def fold_vgg(bank, prefix):
    """Fold eval-mode BatchNorm into the preceding conv: returns [(w, b)] for the 8 VGG-11 convs
    (reference pretrain_models.py:86-104; BN eps 1e-5, running statistics)."""
    out = []
    for i in specs.VGG11_BN_CONVS:
        w, b = bank.p(f"{prefix}.{i}.weight"), bank.p(f"{prefix}.{i}.bias")
        g, beta = bank.p(f"{prefix}.{i + 1}.weight"), bank.p(f"{prefix}.{i + 1}.bias")
        mu, var = bank.p(f"{prefix}.{i + 1}.running_mean"), bank.p(f"{prefix}.{i + 1}.running_var")
        s = g / torch.sqrt(var + 1e-5)
        out.append(((w * s.view(-1, 1, 1, 1)).contiguous(), ((b - mu) * s + beta).contiguous()))
    return out


def range_guarded(nets, fn, recompute=None):
    """fn() over the networks `nets` (None entries skipped), then their range records checked (ParamBank.range_check): the networks whose
    pair maps left the window run `recompute` (default fn) once more with their pair routes off.  The records are cleared first, so maps
    from earlier unchecked calls (captured graphs) do not count against this one."""
    nets = [n for n in nets if n is not None]
    for n in nets:
        t = n.__dict__.get("_range")
        if t is not None and t.names:
            t.clear()
    out = fn()
    left = [n for n in nets if n.range_check()]
    if left:
        for n in left:
            n._range_fallback()
            n._pairs_off = True
        try:
            out = (recompute or fn)()
        finally:
            for n in left:
                n._pairs_off = False
    return out

