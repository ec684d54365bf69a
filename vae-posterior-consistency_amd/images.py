"""When a packed weight image is current: the one rule every model and trainer follows.

A kernel reads the weights from an image packed from the flat parameter buffer (fp32 encoder / decoder images, the bf16
forms).  An image is current while the model's parameter key is the one it was packed at.  The key holds the flat
buffer's address and version, every trainable tensor's version and a per-model generation: writes that torch counts
(`p.mul_()` under no_grad, `load_state_dict`, `flat.copy_()`) change a version by themselves; after every write that
torch does not count (`p.data` writes, a kernel writing `_flat`: each Adam form, a graph replay, a broadcast) the writer
calls `model.invalidate_images()`, which bumps the generation.  A launch that also re-packed images in place then stamps
those with the new key (flat_written).
"""


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
