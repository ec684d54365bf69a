"""When a packed weight image is current: the one rule every model and trainer follows.

A kernel reads the weights from an image packed from the flat parameter buffer (fp32 encoder / decoder images, the bf16
forms).  An image is current while the model's parameter key is the one it was packed at.  The key holds the flat
buffer's address and version, every trainable tensor's version and a per-model generation: writes that torch counts
(`p.mul_()` under no_grad, `load_state_dict`, `flat.copy_()`) change a version by themselves; after every write that
torch does not count (`p.data` writes, a kernel writing `_flat`: each Adam form, a graph replay, a broadcast) the writer
calls `model.invalidate_images()`, which bumps the generation.  A launch that also re-packed images in place then stamps
those with the new key (flat_written).

FlatParams (below) is the flat buffer itself: every model class lays its trainable tensors out through it.
"""
import torch

from ._lib import require_cuda


class ParamKeyMixin:
    _img_gen = 0

    def _param_key(self, params=None):
        """The parameter key (generation first).  `params`: the model's trainable() list, when the caller holds it."""
        flat = self.__dict__.get("_flat")
        ps = self.trainable() if params is None else params
        return (self._img_gen, None if flat is None else flat.data_ptr(), None if flat is None else flat._version,
                *[p._version for p in ps])

    def invalidate_images(self):
        """Every packed image of this model, the trainers' included, is re-packed before its next use."""
        self.__dict__["_img_gen"] = self._img_gen + 1  # (past nn.Module.__setattr__: once per step on host-paced paths)


def mlp_spec(names, module, segment):
    """_flat_spec entries of an nn.Sequential of Linear layers at indices 0, 2, 4, ..: names = (W1, b1, W2, b2, ..)."""
    return tuple((n, f"{module}.{i - i % 2}.{'bias' if i % 2 else 'weight'}", segment) for i, n in enumerate(names))


class FlatParams(ParamKeyMixin):
    """One flat fp32 buffer under a model's trainable tensors, driven by one table per class:

        _flat_spec     ((name, parameter path, segment[, view shape]), ..) in flat-buffer order (= Adam-state order)
        _flat_aliases  {name: (first, .., last)}: adjacent entries joined along rows into ONE GEMM operand

    `trainable()`, the per-segment parameter tuples and sizes, the named views of any buffer laid out like the flat one
    (the parameters themselves, a gradient) all come from that table."""
    _flat_spec = ()
    _flat_aliases = {}

    def _resolve(self, path):
        *mods, leaf = path.split(".")
        m = self
        for k in mods:
            m = m._modules[k]
        return m._parameters[leaf]

    def _flat_table(self):
        """(names, parameters, {segment: (first index, end index, first float, floats)}).  Cached: nn.Module attribute
        lookups are a visible share of a host-paced step; .to() / load_state_dict keep the Parameter objects, and a
        replaced first Parameter drops the cache."""
        c = self.__dict__.get("_table_cache")
        spec = self._flat_spec
        if c is None or c[1][0] is not self._resolve(spec[0][1]):
            ps = [self._resolve(s[1]) for s in spec]
            segs, off = {}, 0
            for i, (s, p) in enumerate(zip(spec, ps)):
                lo = segs.get(s[2], (i, i, off, 0))
                segs[s[2]] = (lo[0], i + 1, lo[2], lo[3] + p.numel())
                off += p.numel()
            c = ([s[0] for s in spec], ps, segs)
            self.__dict__["_table_cache"] = c
            # per entry (name, floats, view shape or None = the flat slice as it is): what _segment_views needs, without a
            # Parameter attribute lookup (1 - 2 us each) per call
            self.__dict__["_split_cache"] = [(s[0], p.numel(), s[3] if len(s) > 3 else None if p.dim() == 1 else tuple(p.shape))
                                             for s, p in zip(spec, ps)]
        return c

    def trainable(self):
        """The trainable tensors in flat-buffer order."""
        return self._flat_table()[1]

    def _segment_params(self, which):
        _, ps, segs = self._flat_table()
        return tuple(ps[segs[which][0]:segs[which][1]])

    def _segment_names(self, which):
        names, _, segs = self._flat_table()
        return names[segs[which][0]:segs[which][1]]

    def _enc_weights(self):
        return self._segment_params("enc")

    def _dec_weights(self):
        return self._segment_params("dec")

    @property
    def _n_enc(self):
        return self._flat_table()[2]["enc"][3]

    @property
    def _n_dec(self):
        return self._flat_table()[2]["dec"][3]

    def flatten_parameters(self):
        """Make the trainable tensors views of ONE flat fp32 buffer (table order).  Idempotent; call again after
        .to(device) / parameter re-assignment (in-place loads keep the buffer).  Returns the flat buffer."""
        ps = self.trainable()
        flat = self.__dict__.get("_flat")
        # fast path: first and last parameter still sit where the flat buffer puts them
        if flat is not None and ps[0].data_ptr() == flat.data_ptr() and \
                ps[-1].data_ptr() == flat.data_ptr() + 4 * (flat.numel() - ps[-1].numel()) and flat.device == ps[0].device:
            return flat
        off = 0
        ok = flat is not None and flat.device == ps[0].device
        if ok:
            for p in ps:
                if p.data.data_ptr() != flat.data_ptr() + 4 * off or not p.data.is_contiguous():
                    ok = False
                    break
                off += p.numel()
        if not ok:
            flat = torch.cat([p.data.detach().reshape(-1).float() for p in ps]).contiguous()
            off = 0
            for p in ps:
                p.data = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
            self._flat = flat
            self.__dict__["_view_cache"] = None
            self.invalidate_images()
        return self._flat

    def _segment_views(self, buf, which):
        """Named views into a buffer laid out like segment `which` of the flat buffer (+ the aliases inside it)."""
        lo, hi = self._flat_table()[2][which][:2]
        ent, out = self.__dict__["_split_cache"][lo:hi], {}
        # (ONE split, and a view only where the shape is not the slice's: the API path makes these per backward call, and a
        # Python slice + view + three Parameter lookups per tensor were 40 us of host time for six tensors)
        for (name, _, shape), t in zip(ent, buf.split([e[1] for e in ent])):
            out[name] = t if shape is None else t.view(shape)
        for name, parts in self._flat_aliases.items():
            if parts[0] in out:
                first = out[parts[0]]
                o = first.storage_offset() - buf.storage_offset()
                rows = sum(out[k].shape[0] for k in parts)
                out[name] = buf[o:o + sum(out[k].numel() for k in parts)].view(rows, *first.shape[1:])
        return out

    def _named_views(self, buf):
        """Every segment's named views of a buffer laid out like the whole flat buffer (a trainer's gradient)."""
        out = {}
        for which, (_, _, lo, n) in self._flat_table()[2].items():
            out.update(self._segment_views(buf[lo:lo + n], which))
        return out

    def _views(self):
        """Named views of the flat parameters (cached per buffer; the steady-state cost is flatten_parameters' pointer check)."""
        flat = self.flatten_parameters()
        vc = self.__dict__.get("_view_cache")
        if vc is None or vc[0] is not flat:
            require_cuda(flat)
            vc = self.__dict__["_view_cache"] = (flat, self._named_views(flat))
        return vc[1]

    def _chains(self):
        """(encoder chain, decoder chain) of linear.py over the flat parameters: the class's _build_chains(views), built once
        per flat buffer (the API path walks them in every forward and backward call)."""
        v = self._views()
        vc = self.__dict__["_view_cache"]
        if len(vc) == 2:
            vc = self.__dict__["_view_cache"] = (*vc, self._build_chains(v))
        return vc[2]


def flat_written(model, params, key, repacked=()):
    """A launch wrote `model._flat` behind torch's back and re-packed the images `repacked` in place.  `key`: the parameter
    key from before the launch, or None."""
    model.invalidate_images()
    if repacked:
        key = (model._img_gen,) + key[1:] if key is not None else model._param_key(params)
        for im in repacked:
            im.stamp(key)


class PackedImage:
    """A device buffer, its pack function `pack(flat, buf)` and the parameter key it was packed at.  The pack function
    holds no reference to the model or the trainer: a trainer that holds a captured graph is then freed by its reference
    count, never by a garbage collection that may run while another graph is being captured."""

    def __init__(self, buf, pack):
        self.buf, self.pack, self.key = buf, pack, None

    def get(self, key, flat):
        if key != self.key:
            self.pack(flat, self.buf)
            self.key = key
        return self.buf

    def stamp(self, key):
        self.key = key
