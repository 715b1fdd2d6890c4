"""Observation augmentations on the learner path (reference: augmentations.py).

``RandomCrop`` keeps the reference's host-side NumPy index stream (the crop
offsets are drawn with ``np.random.randint`` exactly as augmentations.py:66-67
does, so a seeded run picks the same windows); the pixel movement itself is
fused into the first conv kernel's load (curla_amd/csrc/conv.hip) or, for
callers that want tensors, done by ``curla_crop_nchw``.

Every class also tells ``ReplayBuffer`` how a minibatch of its kind is sampled (``sample_kind`` and the methods listed
at ``IdentityAugmentation``; DESIGN.md, "Adding an augmentation"): the buffer asks the object, never what class it is.
"""
import numpy as np
import torch

from . import ops


def _device_batch(image_batch, input_shape):
    """The float NCHW device tensor the augmentation kernels take; anything else is an error (no CPU path)."""
    if not (torch.is_tensor(image_batch) and image_batch.dim() == 4 and image_batch.shape[1] % 3 == 0
            and tuple(image_batch.shape[2:]) == tuple(input_shape)):
        raise ValueError("expected a (B, 3*frame_stack, %d, %d) tensor, got %r"
                         % (input_shape[0], input_shape[1], getattr(image_batch, "shape", type(image_batch))))
    from . import _lib
    if not image_batch.is_cuda and _lib._trace_hook is None:
        raise RuntimeError("ColorJiggle / NoisyCover / RandomConv run on the HIP device only: curla_amd has no CPU path")
    return image_batch.float().contiguous()


class IdentityAugmentation:
    """augmentations.py:7-17."""

    def __init__(self, input_shape):
        assert len(input_shape) == 2, "Input shape must be 2D"
        self.input_shape = tuple(input_shape)
        self.output_shape = tuple(input_shape)

    def evaluation_augmentation(self, image):
        return image

    def training_augmentation(self, image_batch):
        return image_batch

    # ---- what ReplayBuffer asks of an augmentation.  Every class states its ``sample_kind``:
    #   "ring"     nothing is launched: the first conv layer gathers the stored frames and crops ``output_shape``
    #   "scratch"  ONE launch, ``scratch_launch(ring, rows, period, words, n, out)``, writes n uint8 frames of
    #              ``output_shape`` into the sample slot's scratch, which is then read as a ring with zero offsets;
    #              sample s is row rows[s % period] (rows None: s % period), ``words`` its ``index_rows`` int32 runs [n]
    #   "float"    one launch per tensor, ``launch(ring, rows, B, out, staged=None)``, into float NHWC ``out``; it draws
    #              and uploads its parameters itself (one pinned block, one asynchronous copy) unless ``staged`` hands
    #              them over.  With ``staged_aug`` they travel in the minibatch's block instead, ``staged_layout(B,
    #              obs_shape)`` -> (bytes per tensor, the block_layout keys of the fields inside them): ``draw_staged(B,
    #              obs_shape, noise_generator)`` draws one tensor's, ``fill_staged(host, at, drawn)`` writes them at byte
    #              ``at`` of a host copy of the block and ``staged_args(dev, at, B, obs_shape)`` reads ``staged`` back
    #              from there in the device copy.
    # Any kind may draw ``index_rows`` (0, 2, 4 or 6) int32 words per sample and tensor on the host,
    # ``draw_index_words(n)``: the first two travel as the block's offset rows, the others behind them (block_layout: ``cut``).
    index_rows = 0

    @property
    def sample_kind(self):
        """The identity is a "ring"; a subclass inherits no kind from it -- it declares its own (the classes below do, and
        their subclasses inherit that) or is unknown to ReplayBuffer (None: draw_indices raises)."""
        return "ring" if type(self) is IdentityAugmentation else None

    def draw_index_words(self, n):
        """``index_rows`` integer arrays [n], drawn from NumPy's global stream for one tensor of a minibatch."""
        return ()

    def check_staged(self, n, noise_generator):
        """("float") ValueError when ``staged_aug`` cannot serve minibatch tensors of n elements."""


class RandomCrop(IdentityAugmentation):
    """augmentations.py:20-75.  ``output_shape`` may be given explicitly (the
    reference hard-codes ceil(0.84 * side), which maps 84 -> 71; BASELINE.json's
    84 -> 76 needs the override)."""

    def __init__(self, input_shape, output_shape=None):
        super().__init__(input_shape)
        self.cropping_factor = 0.84
        if output_shape is None:
            output_shape = tuple(int(np.ceil(x * self.cropping_factor)) for x in self.input_shape)
        self.output_shape = tuple(output_shape)

    def evaluation_augmentation(self, image):
        """Center crop of a (C, H, W) image (augmentations.py:26-45)."""
        h, w = self.input_shape
        new_h, new_w = self.output_shape
        top = (h - new_h) // 2
        left = (w - new_w) // 2
        return image[:, top:top + new_h, left:left + new_w]

    def draw_offsets(self, n):
        """The two RNG draws of training_augmentation (augmentations.py:66-67):
        h1 then w1, upper bounds exclusive."""
        crop_max_h = self.input_shape[0] - self.output_shape[0]
        crop_max_w = self.input_shape[1] - self.output_shape[1]
        h1 = np.random.randint(0, crop_max_h, n)
        w1 = np.random.randint(0, crop_max_w, n)
        return h1, w1

    sample_kind, index_rows = "ring", 2

    def draw_index_words(self, n):
        return self.draw_offsets(n)

    def training_augmentation(self, image_batch):
        """Host-side crop of a (B, C, H, W) array, for callers outside the fused
        path (same result as augmentations.py:47-75: out[b] = in[b, :, h1:h1+h, w1:w1+w])."""
        n = image_batch.shape[0]
        h1, w1 = self.draw_offsets(n)
        oh, ow = self.output_shape
        out = np.empty(image_batch.shape[:2] + (oh, ow), dtype=image_batch.dtype)
        for b in range(n):
            out[b] = image_batch[b, :, h1[b]:h1[b] + oh, w1[b]:w1[b] + ow]
        return out


class RandomShift(IdentityAugmentation):
    """Beyond the reference: the random shift of DrQ / DrQ-v2.  Every frame is padded by ``pad`` pixels on each side
    with its edge pixels repeated, then a window of the ORIGINAL size is cut at a random offset (dy, dx) in
    [0, 2 pad]^2, one draw per sample shared by all channels of the stack:
        out[c][y][x] = in[c][clamp(y + dy - pad, 0, H - 1)][clamp(x + dx - pad, 0, W - 1)]
    The full field of view and the frame size are kept (``output_shape == input_shape``; not a ``RandomCrop``: nothing
    is centre-cropped at evaluation time).  On the learner path the pixels are moved by ``curla_random_shift_u8`` and
    stay uint8 (ReplayBuffer); the offsets are drawn on the host from NumPy's global stream, like RandomCrop's."""

    def __init__(self, input_shape, pad=4):
        super().__init__(input_shape)
        if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 0:
            raise ValueError("RandomShift: pad must be an int >= 0, got %r" % (pad,))
        self.pad = int(pad)

    def draw_offsets(self, n):
        """Two RNG draws, dy then dx, each in [0, 2 pad] (in the style of RandomCrop.draw_offsets)."""
        dy = np.random.randint(0, 2 * self.pad + 1, n)
        dx = np.random.randint(0, 2 * self.pad + 1, n)
        return dy, dx

    sample_kind, index_rows = "scratch", 2

    def draw_index_words(self, n):
        return self.draw_offsets(n)

    def scratch_launch(self, ring, rows, period, words, n, out):
        dy, dx = words
        ops.random_shift_u8(ring, rows, period, dy, dx, self.pad, n, out)

    def shift(self, image_batch, dy, dx):
        """The shift of a (B, C, H, W) array by given per-sample offsets, on the host."""
        h, w = image_batch.shape[2:]
        out = np.empty_like(image_batch)
        for b in range(image_batch.shape[0]):
            ys = np.clip(np.arange(h) + int(dy[b]) - self.pad, 0, h - 1)
            xs = np.clip(np.arange(w) + int(dx[b]) - self.pad, 0, w - 1)
            out[b] = image_batch[b][:, ys[:, None], xs[None, :]]
        return out

    def training_augmentation(self, image_batch):
        """Host-side shift of a (B, C, H, W) NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        dy, dx = self.draw_offsets(image_batch.shape[0])
        return self.shift(image_batch, dy, dx)


class RandomCutout(IdentityAugmentation):
    """Beyond the reference: the cutout (``color=False``) and cutout-color (``color=True``) of RAD.  One box per sample,
    shared by all frames of the stack, is painted black or in one random RGB colour onto an otherwise untouched frame:
        out[c][y][x] = colour[c % 3]   if y0 <= y < y0 + bh and x0 <= x < x0 + bw,   in[c][y][x] otherwise
    with bh, bw in [min_cut, max_cut] and the box always inside the frame (``output_shape == input_shape``; evaluation
    is the identity).  This is a clean restatement, not a port: RAD's own code reuses one draw for both the position and
    the size of its box, a quirk that is not reproduced here.  On the learner path the boxes are painted by
    ``curla_cutout_u8`` and the minibatch stays uint8 (ReplayBuffer); boxes and colours are drawn on the host from
    NumPy's global stream."""

    def __init__(self, input_shape, min_cut=10, max_cut=30, color=False):
        super().__init__(input_shape)
        for name, v in (("min_cut", min_cut), ("max_cut", max_cut)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("RandomCutout: %s must be an int, got %r" % (name, v))
        # (bh | bw << 16 travels as one non-negative int32 of the minibatch's block: a side has 15 bits)
        if not 1 <= min_cut <= max_cut <= min(min(self.input_shape), 0x7FFF):
            raise ValueError("RandomCutout: need 1 <= min_cut <= max_cut <= min(H, W), got min_cut=%r max_cut=%r for %r"
                             % (min_cut, max_cut, self.input_shape))
        self.min_cut, self.max_cut, self.color = int(min_cut), int(max_cut), bool(color)

    def draw_boxes(self, n):
        """The RNG draws of n boxes, in this order: bh, bw in [min_cut, max_cut], then y0 in [0, H - bh] and x0 in
        [0, W - bw] (array upper bounds), then -- ``color=True`` only -- rgb in [0, 255], shape (n, 3).  Returns
        (y0, x0, bh, bw, rgb); rgb is None for the black cutout, which draws nothing for it."""
        h, w = self.input_shape
        bh = np.random.randint(self.min_cut, self.max_cut + 1, n)
        bw = np.random.randint(self.min_cut, self.max_cut + 1, n)
        y0 = np.random.randint(0, h - bh + 1)
        x0 = np.random.randint(0, w - bw + 1)
        rgb = np.random.randint(0, 256, (n, 3)) if self.color else None
        return y0, x0, bh, bw, rgb

    sample_kind, index_rows = "scratch", 4

    def draw_index_words(self, n):
        """``draw_boxes(n)`` as the kernel takes it: y0, x0, the packed sizes bh | bw << 16 and the colour words
        r | g << 8 | b << 16 (0 for the black cutout)."""
        y0, x0, bh, bw, rgb = self.draw_boxes(n)
        return y0, x0, bh | (bw << 16), 0 if rgb is None else rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)

    def scratch_launch(self, ring, rows, period, words, n, out):
        y0, x0, size, rgb = words
        ops.cutout_u8(ring, rows, period, y0, x0, size, rgb, n, out)

    @staticmethod
    def cut(image_batch, y0, x0, bh, bw, rgb=None):
        """The cutout of a (B, C, H, W) array with given per-sample boxes, on the host; ``rgb`` (B, 3) or None = black."""
        out = np.array(image_batch, copy=True)
        chan = np.arange(out.shape[1]) % 3
        for b in range(out.shape[0]):
            colour = np.zeros(3, dtype=out.dtype) if rgb is None else np.asarray(rgb[b]).astype(out.dtype)
            out[b, :, int(y0[b]):int(y0[b]) + int(bh[b]), int(x0[b]):int(x0[b]) + int(bw[b])] = colour[chan][:, None, None]
        return out

    def training_augmentation(self, image_batch):
        """Host-side cutout of a (B, C, H, W) NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        return self.cut(image_batch, *self.draw_boxes(image_batch.shape[0]))


class RandomTranslate(IdentityAugmentation):
    """Beyond the reference: the translate of RAD.  The H x W frame is placed at a random position (ty, tx) on a black
    canvas of ``output_shape = (Ho, Wo)`` (``None``: (H + 8, W + 8), a margin of 4 per side like RandomShift's default
    pad), one draw per sample shared by all channels of the stack:
        out[c][y][x] = in[c][y - ty][x - tx]   if 0 <= y - ty < H and 0 <= x - tx < W,   0 otherwise
    with ty in [0, Ho - H] and tx in [0, Wo - W].  Every source pixel is kept and none is invented; the minibatch frame is
    LARGER than the stored frame, and the encoder is built for (C, Ho, Wo).  Evaluation centres the frame on the canvas.
    A clean restatement of RAD's ``random_translate`` / ``center_translate``, not a port.  On the learner path the pixels
    are moved by ``curla_translate_u8`` and stay uint8 (ReplayBuffer); the offsets are drawn on the host from NumPy's
    global stream, like RandomCrop's."""

    def __init__(self, input_shape, output_shape=None):
        for name, shape in (("input_shape", input_shape), ("output_shape", output_shape)):
            if shape is None:
                continue
            if len(shape) != 2:
                raise ValueError("RandomTranslate: %s must be 2D, got %r" % (name, shape))
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in shape):
                raise ValueError("RandomTranslate: %s must hold ints, got %r" % (name, shape))
        if output_shape is None:
            output_shape = tuple(x + 8 for x in input_shape)
        super().__init__(tuple(int(x) for x in input_shape))
        self.output_shape = tuple(int(x) for x in output_shape)
        if self.output_shape[0] < self.input_shape[0] or self.output_shape[1] < self.input_shape[1]:
            raise ValueError("RandomTranslate: the canvas %r must be no smaller than the frame %r"
                             % (self.output_shape, self.input_shape))

    def draw_offsets(self, n):
        """Two RNG draws, ty then tx, in [0, Ho - H] and [0, Wo - W] (in the style of RandomShift.draw_offsets)."""
        ty = np.random.randint(0, self.output_shape[0] - self.input_shape[0] + 1, n)
        tx = np.random.randint(0, self.output_shape[1] - self.input_shape[1] + 1, n)
        return ty, tx

    sample_kind, index_rows = "scratch", 2

    def draw_index_words(self, n):
        return self.draw_offsets(n)

    def scratch_launch(self, ring, rows, period, words, n, out):
        ty, tx = words
        ops.translate_u8(ring, rows, period, ty, tx, n, out)

    def translate(self, image_batch, ty, tx):
        """A (B, C, H, W) array placed at given per-sample offsets on zero canvases (B, C, Ho, Wo), on the host."""
        h, w = image_batch.shape[2:]
        out = np.zeros(image_batch.shape[:2] + self.output_shape, dtype=image_batch.dtype)
        for b in range(image_batch.shape[0]):
            out[b, :, int(ty[b]):int(ty[b]) + h, int(tx[b]):int(tx[b]) + w] = image_batch[b]
        return out

    def training_augmentation(self, image_batch):
        """Host-side translate of a (B, C, H, W) NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        ty, tx = self.draw_offsets(image_batch.shape[0])
        return self.translate(image_batch, ty, tx)

    def evaluation_augmentation(self, image):
        """A (C, H, W) image centred on a zero canvas (C, Ho, Wo) of its dtype (an odd margin leaves the larger part
        below / to the right); an image that already has the canvas size is returned as it is."""
        if tuple(image.shape[-2:]) == self.output_shape:
            return image
        h, w = image.shape[-2:]
        top, left = (self.output_shape[0] - h) // 2, (self.output_shape[1] - w) // 2
        out = np.zeros(tuple(image.shape[:-2]) + self.output_shape, dtype=image.dtype)
        out[..., top:top + h, left:left + w] = image
        return out


def _checked_hw_p(name, input_shape, p):
    """(input_shape as a tuple of two ints, p as a float): what RandomFlip, RandomRotate and RandomGrayscale validate alike."""
    if len(input_shape) != 2:
        raise ValueError("%s: input_shape must be 2D, got %r" % (name, input_shape))
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in input_shape):
        raise ValueError("%s: input_shape must hold ints, got %r" % (name, input_shape))
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("%s: p must be a number in [0, 1], got %r" % (name, p))
    return tuple(int(x) for x in input_shape), float(p)


FLIP_X, FLIP_Y, TRANSPOSE = 1, 2, 4  # the bits of a dihedral code (curla_dihedral_u8)
ROT90_CODES = (0, FLIP_X | TRANSPOSE, FLIP_X | FLIP_Y, FLIP_Y | TRANSPOSE)  # of np.rot90(k = 0, 1, 2, 3) over (H, W)


def dihedral(image_batch, codes):
    """The map of ``curla_dihedral_u8`` on a (B, C, H, W) array, on the host: with (a, b) = (x, y) if the TRANSPOSE bit of
    codes[b] is set, else (y, x), out[c][y][x] = in[c][FLIP_Y ? H - 1 - a : a][FLIP_X ? W - 1 - b : b]."""
    image_batch = np.asarray(image_batch)
    out = np.empty_like(image_batch)
    for b in range(image_batch.shape[0]):
        img, code = image_batch[b], int(codes[b])
        if code & FLIP_Y:
            img = img[:, ::-1]
        if code & FLIP_X:
            img = img[:, :, ::-1]
        out[b] = img.transpose(0, 2, 1) if code & TRANSPOSE else img
    return out


class RandomFlip(IdentityAugmentation):
    """Beyond the reference: the flip of RAD.  A sample is mirrored left-right with probability ``p``, one draw per sample
    shared by all frames of the stack:
        out[c][y][x] = in[c][y][W - 1 - x]   if flipped,   in[c][y][x] otherwise
    ``output_shape == input_shape``; evaluation is the identity.  A clean restatement of RAD's ``random_flip``, not a
    port.  On the learner path the pixels are moved by ``curla_dihedral_u8`` (code 1 or 0) and stay uint8 (ReplayBuffer);
    the flags are drawn on the host from NumPy's global stream, one ``np.random.rand(n) < p`` per tensor."""

    def __init__(self, input_shape, p=0.5):
        shape, self.p = _checked_hw_p("RandomFlip", input_shape, p)
        super().__init__(shape)

    def draw_flags(self, n):
        """One RNG call: ``np.random.rand(n) < p``."""
        return np.random.rand(n) < self.p

    sample_kind, index_rows = "scratch", 2

    def draw_index_words(self, n):
        """(code, 0): 1 where the sample is flipped, 0 where it is not; the second word is not used."""
        return self.draw_flags(n).astype(np.int32) * FLIP_X, 0

    def scratch_launch(self, ring, rows, period, words, n, out):
        ops.dihedral_u8(ring, rows, period, words[0], n, out)

    @staticmethod
    def flip(image_batch, flags):
        """A (B, C, H, W) array with the samples whose flag is set mirrored left-right, on the host."""
        out = np.array(image_batch, copy=True)
        for b in range(out.shape[0]):
            if flags[b]:
                out[b] = out[b, :, :, ::-1]
        return out

    def training_augmentation(self, image_batch):
        """Host-side flip of a (B, C, H, W) NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        return self.flip(image_batch, self.draw_flags(image_batch.shape[0]))


class RandomRotate(IdentityAugmentation):
    """Beyond the reference: the rotate of RAD.  With probability ``p`` (RAD's default 0.3) a sample is turned by a random
    multiple of 90 degrees, counter-clockwise as ``np.rot90`` over (H, W) turns, one draw per sample shared by all frames
    of the stack; a frame that is not square is turned by 0 or 180 degrees only, which keep its size.
    ``output_shape == input_shape``; evaluation is the identity.  A clean restatement of RAD's ``random_rotation``, not a
    port.  On the learner path the pixels are moved by ``curla_dihedral_u8`` (codes 0, 5, 3, 6 for k = 0, 1, 2, 3) and stay
    uint8 (ReplayBuffer); the turns are drawn on the host from NumPy's global stream."""

    def __init__(self, input_shape, p=0.3):
        shape, self.p = _checked_hw_p("RandomRotate", input_shape, p)
        super().__init__(shape)

    def draw_turns(self, n):
        """Two RNG calls, always both and in this order: ``turns = np.random.randint(0, 4, n)`` on a square frame,
        ``2 * np.random.randint(0, 2, n)`` on any other; then ``keep = np.random.rand(n) < p``.  Returns k = turns where
        keep, else 0."""
        if self.input_shape[0] == self.input_shape[1]:
            turns = np.random.randint(0, 4, n)
        else:
            turns = 2 * np.random.randint(0, 2, n)
        keep = np.random.rand(n) < self.p
        return np.where(keep, turns, 0)

    sample_kind, index_rows = "scratch", 2

    def draw_index_words(self, n):
        """(code, 0): the dihedral code of each sample's k; the second word is not used."""
        return np.asarray(ROT90_CODES, dtype=np.int32)[self.draw_turns(n)], 0

    def scratch_launch(self, ring, rows, period, words, n, out):
        ops.dihedral_u8(ring, rows, period, words[0], n, out)

    @staticmethod
    def rotate(image_batch, k):
        """A (B, C, H, W) array with sample b turned k[b] times by 90 degrees counter-clockwise, on the host (odd k[b] on
        square frames only)."""
        return dihedral(image_batch, [ROT90_CODES[int(t) % 4] for t in k])

    def training_augmentation(self, image_batch):
        """Host-side rotation of a (B, C, H, W) NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        return self.rotate(image_batch, self.draw_turns(image_batch.shape[0]))


class RandomGrayscale(IdentityAugmentation):
    """Beyond the reference: the grayscale of RAD.  With probability ``p`` (RAD's default 0.3) every RGB frame of a sample
    loses its colour, one draw per sample shared by all frames of the stack: each triplet (R, G, B) becomes (g, g, g),
        g = (77 R + 150 G + 29 B + 128) >> 8
    an integer mix within 1 of RAD's 0.2989 R + 0.587 G + 0.114 B whose weights sum to 256 -- a grey pixel stays what it
    is, so the map is idempotent.  ``output_shape == input_shape``; evaluation is the identity.  A clean restatement of
    RAD's ``random_grayscale``, not a port.  On the learner path the bytes are mixed by ``curla_grayscale_u8`` and stay
    uint8 (ReplayBuffer); the flags are drawn on the host from NumPy's global stream, one ``np.random.rand(n) < p`` per
    tensor.  The channel count is no part of ``input_shape``: one that is no multiple of 3 is refused where it is first
    seen -- by ``grey`` on the host, by ``ops.grayscale_u8`` and by the kernel on the learner path, before any launch."""

    def __init__(self, input_shape, p=0.3):
        shape, self.p = _checked_hw_p("RandomGrayscale", input_shape, p)
        super().__init__(shape)

    def draw_flags(self, n):
        """One RNG call: ``np.random.rand(n) < p``."""
        return np.random.rand(n) < self.p

    sample_kind, index_rows = "scratch", 2

    def draw_index_words(self, n):
        """(flag, 0): 1 where the sample is greyed, 0 where it is not; the second word is not used."""
        return self.draw_flags(n).astype(np.int32), 0

    def scratch_launch(self, ring, rows, period, words, n, out):
        ops.grayscale_u8(ring, rows, period, words[0], n, out)

    @staticmethod
    def grey(image_batch, flags):
        """A (B, 3k, H, W) uint8 array with the samples whose flag is set greyed, on the host: the integer formula of the
        class docstring."""
        out = np.array(image_batch, copy=True)
        B, C, H, W = out.shape
        if C % 3:
            raise ValueError("RandomGrayscale: the channels must be RGB triplets, got %d channels" % C)
        x = out.reshape(B, C // 3, 3, H, W).astype(np.int64)
        g = ((77 * x[:, :, 0] + 150 * x[:, :, 1] + 29 * x[:, :, 2] + 128) >> 8).astype(out.dtype)
        for b in range(B):
            if flags[b]:
                out[b] = np.repeat(g[b], 3, axis=0)
        return out

    def training_augmentation(self, image_batch):
        """Host-side greyscale of a (B, 3k, H, W) uint8 NumPy array, for callers outside the fused path."""
        image_batch = np.asarray(image_batch)
        return self.grey(image_batch, self.draw_flags(image_batch.shape[0]))


def _finite_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(float(v)))


class RandomAffine(IdentityAugmentation):
    """Beyond the reference: the rotate / zoom / sub-pixel shift of kornia's and torchvision's ``RandomAffine`` -- the one
    augmentation of the uint8 path that RESAMPLES.  A sample is turned by theta in [-degrees, degrees] (positive: counter-
    clockwise, as ``np.rot90`` turns) about the frame's centre, zoomed by s in ``scale`` and shifted by (ty, tx) in
    ``translate`` * (H, W) pixels, one draw per sample shared by all frames of the stack, with probability ``p``; pixels
    from outside the frame repeat the edge (``fill='edge'``) or are black (``fill='zero'``).  ``output_shape ==
    input_shape``; evaluation is the identity.  The map is defined in integers, so that the device, this file and the
    tests agree bit for bit: six int32 words per sample, a 16.16 fixed-point INVERSE map from output pixel (y, x) to source
    coordinates,
        X = wrap32(m00 x + m01 y + m02)        Y = wrap32(m10 x + m11 y + m12)
        x0 = X >> 16 (floor)   fx = (X >> 8) & 255          y0 = Y >> 16   fy = (Y >> 8) & 255
        out[c][y][x] = (P(y0, x0)[c] (256 - fx) (256 - fy) + P(y0, x0 + 1)[c] fx (256 - fy)
                      + P(y0 + 1, x0)[c] (256 - fx) fy     + P(y0 + 1, x0 + 1)[c] fx fy     + 32768) >> 16
    with P the source pixel at clamped coordinates (edge) or 0 outside the frame (zero).  With a = cos(theta) / s,
    b = -sin(theta) / s, (cx, cy) = ((W - 1) / 2, (H - 1) / 2) and (ux, uy) = (cx + tx, cy + ty), in float64:
        m00 = rint(65536 a)    m01 = rint(65536 b)    m02 = rint(65536 (cx - a ux - b uy))
        m10 = rint(-65536 b)   m11 = rint(65536 a)    m12 = rint(65536 (cy + b ux - a uy))
    A clean restatement, not a port.  On the learner path the pixels are blended by ``curla_affine_u8`` and stay uint8
    (ReplayBuffer); the parameters are drawn on the host from NumPy's global stream."""

    IDENTITY_WORDS = (65536, 0, 0, 0, 65536, 0)

    def __init__(self, input_shape, degrees=10.0, scale=(0.9, 1.1), translate=0.05, fill='edge', p=1.0):
        shape, self.p = _checked_hw_p("RandomAffine", input_shape, p)
        super().__init__(shape)
        if not _finite_number(degrees) or not 0.0 <= float(degrees) <= 180.0:
            raise ValueError("RandomAffine: degrees must be a finite number in [0, 180], got %r" % (degrees,))
        if (isinstance(scale, (str, bytes)) or not hasattr(scale, "__len__") or len(scale) != 2
                or not all(_finite_number(v) for v in scale) or not 0.0 < float(scale[0]) <= float(scale[1])):
            raise ValueError("RandomAffine: scale must be two finite numbers with 0 < lo <= hi, got %r" % (scale,))
        if not _finite_number(translate) or not 0.0 <= float(translate) <= 0.5:
            raise ValueError("RandomAffine: translate must be a number in [0, 0.5], got %r" % (translate,))
        if not isinstance(fill, str) or fill not in ('edge', 'zero'):
            raise ValueError("RandomAffine: fill must be 'edge' or 'zero', got %r" % (fill,))
        self.degrees, self.scale = float(degrees), (float(scale[0]), float(scale[1]))
        self.translate, self.fill = float(translate), fill
        # (sufficient for no word and no source coordinate of a pixel of the frame to leave 32 bits: |a|, |b| <= g, and
        # the centre plus the shift is at most (0.5 + translate) of a side)
        h, w = self.input_shape
        g = 1.0 / self.scale[0]
        if not 65536.0 * (g * (h + w) * (1.5 + self.translate) + max(h, w) / 2.0 + 1.0) < 2.0 ** 31:
            raise ValueError("RandomAffine: frames of %r at scale >= %r do not fit the 16.16 words of the map"
                             % (self.input_shape, self.scale[0]))

    def draw_params(self, n):
        """Five RNG calls, always all and in this order: ``uniform(-degrees, degrees, n)``, ``uniform(scale[0], scale[1],
        n)``, ``uniform(-translate H, translate H, n)`` (ty), ``uniform(-translate W, translate W, n)`` (tx) and
        ``rand(n) < p``.  Returns (theta in radians, s, ty, tx, keep)."""
        h, w = self.input_shape
        deg = np.random.uniform(-self.degrees, self.degrees, n)
        s = np.random.uniform(self.scale[0], self.scale[1], n)
        ty = np.random.uniform(-self.translate * h, self.translate * h, n)
        tx = np.random.uniform(-self.translate * w, self.translate * w, n)
        keep = np.random.rand(n) < self.p
        return np.deg2rad(deg), s, ty, tx, keep

    def words(self, theta, s, ty, tx):
        """int32 [6][n]: the words m00 m01 m02 m10 m11 m12 of given per-sample parameters (the class docstring's formulas,
        in float64; theta in radians)."""
        theta, s, ty, tx = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (theta, s, ty, tx))
        h, w = self.input_shape
        a, b = np.cos(theta) / s, -np.sin(theta) / s
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        ux, uy = cx + tx, cy + ty
        m = np.stack(np.broadcast_arrays(65536.0 * a, 65536.0 * b, 65536.0 * (cx - a * ux - b * uy),
                                         -65536.0 * b, 65536.0 * a, 65536.0 * (cy + b * ux - a * uy)))
        return np.rint(m).astype(np.int64).astype(np.int32)

    sample_kind, index_rows = "scratch", 6

    def draw_index_words(self, n):
        """The six words of ``draw_params(n)`` in the order m00 ... m12; a sample that is not kept gets the identity's."""
        theta, s, ty, tx, keep = self.draw_params(n)
        m = self.words(theta, s, ty, tx)
        return tuple(np.where(keep, m[k], np.int32(self.IDENTITY_WORDS[k])).astype(np.int32) for k in range(6))

    def scratch_launch(self, ring, rows, period, words, n, out):
        ops.affine_u8(ring, rows, period, words, 1 if self.fill == 'edge' else 0, n, out)

    def warp(self, image_batch, words):
        """The map of ``curla_affine_u8`` on a (B, C, H, W) uint8 array with given per-sample words ([6][B], any
        integers: they are taken modulo 2^32), on the host: the class docstring's formula in int64."""
        img = np.asarray(image_batch)
        B, C, H, W = img.shape

        def wrap32(v):
            return ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31

        m = wrap32(np.stack([np.asarray(w).astype(np.int64).reshape(-1) for w in words]))
        y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
        out = np.empty_like(img)
        for b in range(B):
            X = wrap32(m[0, b] * x + m[1, b] * y + m[2, b])
            Y = wrap32(m[3, b] * x + m[4, b] * y + m[5, b])
            x0, y0, fx, fy = X >> 16, Y >> 16, (X >> 8) & 255, (Y >> 8) & 255
            acc = np.full((C, H, W), 32768, dtype=np.int64)
            for yy, wy in ((y0, 256 - fy), (y0 + 1, fy)):
                for xx, wx in ((x0, 256 - fx), (x0 + 1, fx)):
                    tap = img[b][:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
                    if self.fill == 'zero':
                        tap = tap * ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W))
                    acc += tap * (wx * wy)
            out[b] = (acc >> 16).astype(img.dtype)
        return out

    def training_augmentation(self, image_batch):
        """Host-side warp of a (B, C, H, W) uint8 NumPy array, for callers outside the fused path: ``draw_params``,
        ``words`` (the identity's where a sample is not kept), ``warp``."""
        image_batch = np.asarray(image_batch)
        return self.warp(image_batch, self.draw_index_words(image_batch.shape[0]))


class Compose(IdentityAugmentation):
    """Beyond the reference: a geometric uint8 augmentation followed by a cutout -- RAD's ``crop-cutout_color`` or
    ``translate-cutout`` -- as ONE augmentation.  ``move`` is a RandomCrop, a RandomShift or a RandomTranslate, ``paint`` a
    RandomCutout built for the move's ``output_shape``:
        mid = move(in)                                               (Ho, Wo) = move.output_shape
        out[c][y][x] = colour[c % 3]   if y0 <= y < y0 + bh and x0 <= x < x0 + bw,   mid[c][y][x] otherwise
    with the box in coordinates of the OUTPUT frame; one draw of everything per sample, shared by the frames of a stack:
    first the move's two words, then the paint's four (``RandomCutout.draw_boxes``).  ``input_shape`` / ``output_shape``
    are the move's, and so is evaluation (the cutout's is the identity).  On the learner path the pixels are moved and
    painted by one launch of ``curla_move_cutout_u8`` -- the ring is read once and the scratch written once -- and stay
    uint8 (ReplayBuffer); under a RandomCrop mover the encoder is built for the cropped size, as for a RandomCrop alone."""

    sample_kind, index_rows = "scratch", 6

    def __init__(self, move, paint):
        kinds = ((RandomCrop, ops.MOVE_CROP), (RandomShift, ops.MOVE_SHIFT), (RandomTranslate, ops.MOVE_TRANSLATE))
        code = [c for cls, c in kinds if isinstance(move, cls)]
        if not code:
            raise ValueError("Compose: move must be a RandomCrop, RandomShift or RandomTranslate, got %r" % (move,))
        if not isinstance(paint, RandomCutout):
            raise ValueError("Compose: paint must be a RandomCutout, got %r" % (paint,))
        if tuple(paint.input_shape) != tuple(move.output_shape):
            raise ValueError("Compose: the paint is built for frames of %r, the move makes frames of %r"
                             % (tuple(paint.input_shape), tuple(move.output_shape)))
        self.move, self.paint = move, paint
        self.input_shape, self.output_shape = tuple(move.input_shape), tuple(move.output_shape)
        self._move_code = code[0]

    def draw_index_words(self, n):
        """The move's two words, then the paint's four, drawn in that order."""
        return tuple(self.move.draw_index_words(n)) + tuple(self.paint.draw_index_words(n))

    def scratch_launch(self, ring, rows, period, words, n, out):
        a, b, y0, x0, size, rgb = words
        ops.move_cutout_u8(ring, rows, period, self._move_code, a, b, getattr(self.move, "pad", 0), (y0, x0, size, rgb),
                           n, out)

    def evaluation_augmentation(self, image):
        return self.move.evaluation_augmentation(image)

    def training_augmentation(self, image_batch):
        """Host-side move, then cutout, of a (B, C, H, W) NumPy array, for callers outside the fused path (the draws in
        the order of ``draw_index_words``)."""
        return self.paint.training_augmentation(self.move.training_augmentation(np.asarray(image_batch)))


class RandomConv(IdentityAugmentation):
    """Beyond the reference: the random convolution of RAD (``random_convolution``) and of Lee et al., "Network
    Randomization".  Every sample's RGB frames go through one freshly drawn 3x3, 3 -> 3 channel filter, shared by all
    frames of the stack -- colours and textures change, layout does not:
        out[3 f + co][y][x] = sum over ci, ky, kx of  w[co][ci][ky][kx] * in[3 f + ci][y + ky - 1][x + kx - 1]
    a cross-correlation (no kernel flip) with ``in`` taken as 0 outside the frame.  Input is the stored bytes as floats in
    [0, 255]; the output is float on the same scale and NOT clamped (RAD does not clamp).  ``output_shape ==
    input_shape``; evaluation is the identity.  ``p`` is the probability that a sample is convolved at all (Lee et al. mix
    in clean samples): a sample that is not gets the identity filter, which returns its bytes exactly.  A clean
    restatement, not a port of RAD's code.  On the learner path the frames are convolved straight from the ring by
    ``curla_random_conv`` into the float NHWC minibatch (ReplayBuffer, like ColorJiggle); the weights are drawn on the host
    from torch's CPU generator."""

    def __init__(self, input_shape, p=1.0):
        super().__init__(input_shape)
        if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
            raise ValueError("RandomConv: p must be a number in [0, 1], got %r" % (p,))
        self.p = float(p)

    @staticmethod
    def identity_filter():
        """float32 [3, 3, 3, 3]: w[c][c][1][1] = 1, 0 elsewhere."""
        w = torch.zeros(3, 3, 3, 3, dtype=torch.float32)
        for c in range(3):
            w[c, c, 1, 1] = 1.0
        return w

    def draw_weights(self, n):
        """float32 [n, 3, 3, 3, 3] = w[sample][co][ci][ky][kx] from torch's CPU generator, in this order: first
        ``torch.randn(n, 3, 3, 3, 3) * sqrt(2 / 54)`` (Xavier-normal for fan-in = fan-out = 27, RAD's initialisation);
        then -- ``p < 1`` only -- ``torch.rand(n) < p``, and the rows that lose this draw become the identity filter.
        With ``p == 1`` exactly one generator call is made."""
        w = torch.randn(n, 3, 3, 3, 3, dtype=torch.float32) * np.sqrt(2.0 / 54.0)
        if self.p < 1.0:
            keep = torch.rand(n) < self.p
            w[~keep] = self.identity_filter()
        return w

    sample_kind = "float"

    def staged_layout(self, B, obs_shape):
        """weights float [B][81] | 4 bytes of padding when B is odd (the block stays a multiple of 8 bytes)."""
        return (324 * B + 7) // 8 * 8, dict(aug_weights=324 * B)

    def draw_staged(self, B, obs_shape, noise_generator):
        return self.draw_weights(B)

    def fill_staged(self, host, at, drawn):
        host[at:at + 4 * drawn.numel()].view(torch.float32).copy_(drawn.reshape(-1))

    def staged_args(self, dev, at, B, obs_shape):
        return dev[at:at + 324 * B].view(torch.float32).view(-1, 81)

    def draw_unstaged(self, B, shape, device):
        """What ``launch`` draws for a [B, H, W, C] tensor whose parameters are not staged -- all a positive that nobody
        wants needs (ReplayBuffer.sample_cpc_refs(want_pos=False)): the streams move, nothing is launched."""
        return self.draw_weights(B)

    def launch(self, ring, rows, B, out, staged=None):
        if staged is None:
            weights = self.draw_unstaged(B, out.shape, out.device)
            # (one pinned staging block, one asynchronous copy, as ColorJiggle's)
            stage = torch.empty(weights.shape, dtype=torch.float32, pin_memory=out.is_cuda)
            stage.copy_(weights)
            staged = stage.to(out.device, non_blocking=True)
        ops.random_conv(ring, rows, staged, B, out)

    @staticmethod
    def conv(image_batch, weights):
        """The convolution of a (B, 3k, H, W) array with given per-sample weights (B, 3, 3, 3, 3) (or (B, 81)), on the
        host in float64: the formula of the class docstring, term by term."""
        x = np.asarray(image_batch, dtype=np.float64)
        B, C, H, W = x.shape
        w = np.asarray(weights, dtype=np.float64).reshape(B, 3, 3, 3, 3)
        k = C // 3
        xp = np.zeros((B, k, 3, H + 2, W + 2), dtype=np.float64)
        xp[:, :, :, 1:-1, 1:-1] = x.reshape(B, k, 3, H, W)
        out = np.zeros((B, k, 3, H, W), dtype=np.float64)
        for ky in range(3):
            for kx in range(3):
                out += np.einsum("boc,bfchw->bfohw", w[:, :, :, ky, kx], xp[:, :, :, ky:ky + H, kx:kx + W])
        return out.reshape(B, C, H, W)

    def training_augmentation(self, image_batch, weights=None):
        """On the reference's tensor contract, as ColorJiggle's: a float (B, 3k, H, W) device tensor in [0, 255] in, the
        convolved batch out, always a new tensor (``curla_random_conv_nchw``: the same arithmetic ``ReplayBuffer`` applies
        straight from the ring).  ``weights`` (B, 3, 3, 3, 3) replaces the draw (tests)."""
        x = _device_batch(image_batch, self.input_shape)
        if weights is None:
            weights = self.draw_weights(x.shape[0])
        out = torch.empty_like(x)
        ops.random_conv_nchw(x, torch.as_tensor(weights).to(x.device, torch.float32).contiguous(), out)
        return out


class ColorJiggle(IdentityAugmentation):
    """augmentations.py:78-136: every RGB frame of the stack is jittered independently with probability
    0.85 -- contrast U(0.8,1.2), saturation U(0.5,1.5), hue U(-0.5,0.5) turns, brightness 0 -- the four
    operations applied in one random order per call.

    PARITY UNPINNED: the reference delegates the arithmetic to kornia (not vendored, version un-pinned).
    The arithmetic here (curla_amd/csrc/augment.hip, restated in oracle/curla_oracle.py) follows kornia's
    documented ColorJiggle: brightness additive (0 -> identity), contrast x*c clamped to [0,1], saturation
    and hue through HSV.  Random parameters are drawn on the host from torch's CPU generator."""

    p, contrast, saturation, hue = 0.85, 0.2, 0.5, 0.5

    def draw_params(self, n_images):
        """(params [n_images, 4] = apply, contrast, saturation, hue in radians; order [4])."""
        apply = (torch.rand(n_images) < self.p).float()
        con = torch.empty(n_images).uniform_(1 - self.contrast, 1 + self.contrast)
        sat = torch.empty(n_images).uniform_(1 - self.saturation, 1 + self.saturation)
        hue = torch.empty(n_images).uniform_(-self.hue, self.hue) * (2 * np.pi)
        order = torch.randperm(4).int()
        return torch.stack([apply, con, sat, hue], 1).contiguous(), order

    sample_kind = "float"

    def staged_layout(self, B, obs_shape):
        """params float [B k][4] | order int32 [4]."""
        n_par = 16 * B * (obs_shape[0] // 3)
        return n_par + 16, dict(aug_order=n_par)

    def draw_staged(self, B, obs_shape, noise_generator):
        return self.draw_params(B * (obs_shape[0] // 3))

    def fill_staged(self, host, at, drawn):
        params, order = drawn
        n_par = 4 * params.numel()
        host[at:at + n_par].view(torch.float32).copy_(params.reshape(-1))
        host[at + n_par:at + n_par + 16].view(torch.int32).copy_(order)

    def staged_args(self, dev, at, B, obs_shape):
        n_par = 16 * B * (obs_shape[0] // 3)
        return dev[at:at + n_par].view(torch.float32).view(-1, 4), dev[at + n_par:at + n_par + 16].view(torch.int32)

    def draw_unstaged(self, B, shape, device):
        """What ``launch`` draws for a [B, H, W, C] tensor whose parameters are not staged (RandomConv.draw_unstaged)."""
        return self.draw_params(B * (shape[3] // 3))

    def launch(self, ring, rows, B, out, staged=None):
        if staged is None:
            params, order = self.draw_unstaged(B, out.shape, out.device)
            # one pinned staging block, one asynchronous copy: a `.to(device)` of a pageable tensor makes the host wait
            # until the stream has drained (two of them per call left ~60 us of idle GPU around every jitter launch)
            n4 = params.numel()
            stage = torch.empty(n4 + 4, dtype=torch.int32, pin_memory=out.is_cuda)
            stage[:n4] = params.reshape(-1).view(torch.int32)
            stage[n4:] = order
            d = stage.to(out.device, non_blocking=True)
            staged = d[:n4].view(torch.float32).view(params.shape), d[n4:]
        ops.color_jiggle(ring, rows, staged[0], staged[1], B, out)

    def training_augmentation(self, image_batch, params=None, order=None):
        """augmentations.py:105-136 on the reference's tensor contract: a float (B, 3k, H, W) device tensor in
        [0,255] in, the jittered batch out -- the same kernel arithmetic ``ReplayBuffer`` applies straight from
        the ring.  A new tensor is returned (the reference scales its argument in place by 1/255 and returns a
        fresh tensor; callers only use the return value, utils.py:174-182).  ``params`` / ``order`` replace
        the random draws (tests)."""
        x = _device_batch(image_batch, self.input_shape)
        B, C = x.shape[:2]
        if params is None:
            params, order = self.draw_params(B * (C // 3))
        out = torch.empty_like(x)
        ops.color_jiggle_nchw(x, params.to(x.device, torch.float32).contiguous(),
                              torch.as_tensor(order, dtype=torch.int32).to(x.device), out)
        return out


class NoisyCover(IdentityAugmentation):
    """augmentations.py:138-205: rows [0, ceil(0.31 h)) and [h - ceil(0.20 h), h) of every frame are painted
    with one random colour per RGB channel (np.random.randint(0, 255) x3 per call, shared by the batch),
    Gaussian noise N(0, 10) is added and the result clamped to [0, 255].  Noise: torch generator of the
    device (kornia's RandomGaussianNoise in the reference; PARITY UNPINNED for the noise stream only)."""

    def __init__(self, input_shape):
        super().__init__(input_shape)
        self.h = self.input_shape[0]
        self.top = int(np.ceil(self.h * 0.31))
        self.bottom = int(np.ceil(self.h * 0.20))
        self.std = 10.0

    def draw_colors(self):
        return [np.random.randint(0, 255) for _ in range(3)]

    sample_kind = "float"

    def check_staged(self, n, noise_generator):
        if n >= 2 ** 32:
            raise ValueError("staged_aug: the in-kernel noise numbers a minibatch tensor's elements in 32 bits")
        try:
            noise_generator().get_offset()
        except (AttributeError, RuntimeError) as e:
            raise ValueError("staged_aug=True with NoisyCover draws its noise from the Philox stream of the HIP "
                             f"device's torch generator, which exposes no offset here ({e!r})") from e

    def staged_layout(self, B, obs_shape):
        """colours float [3] | 4 bytes of padding | (seed, Philox counter) uint64 [2], 8-byte aligned."""
        return 32, dict(aug_rng=16)

    def draw_staged(self, B, obs_shape, noise_generator):
        """The colours, and (seed, counter) of the noise the kernel draws: the tensor's ceil(n / 4) Philox counters are
        reserved by moving the device generator's offset on by 4 ceil(n / 4), as CurlSacAgent._noise does."""
        colors = self.draw_colors()
        gen = noise_generator()
        off, n = gen.get_offset(), B * int(np.prod(obs_shape))
        gen.set_offset(off + 4 * ((n + 3) // 4))
        return colors, gen.initial_seed() & (2 ** 64 - 1), off // 4

    def fill_staged(self, host, at, drawn):
        colors, seed, ctr = drawn
        host[at:at + 12].view(torch.float32).copy_(torch.tensor([float(v) for v in colors]))
        host[at + 16:at + 32].view(torch.int64).copy_(
            torch.from_numpy(np.array([seed, ctr], dtype=np.uint64).view(np.int64)))

    def staged_args(self, dev, at, B, obs_shape):
        """Device addresses of the colours and of (seed, counter): the kernel reads both when it runs."""
        return dev.data_ptr() + at, dev.data_ptr() + at + 16

    def draw_unstaged(self, B, shape, device):
        """What ``launch`` draws for a [B, H, W, C] tensor whose parameters are not staged (RandomConv.draw_unstaged):
        the colours and the noise tensor -- torch's own ``randn`` launch, which is what moves the device generator."""
        return self.draw_colors(), torch.randn(tuple(shape), device=device)

    def launch(self, ring, rows, B, out, staged=None):
        if staged is None:
            colors, noise = self.draw_unstaged(B, out.shape, out.device)
            noise = noise * self.std
            ops.noisy_cover(ring, rows, noise, colors, self.top, self.bottom, B, out)
        else:
            ops.noisy_cover_rng(ring, rows, self.std, (0, 0, staged[1]), staged[0], self.top, self.bottom, B, out)

    def training_augmentation(self, image_batch, colors=None, noise=None):
        """augmentations.py:170-205 on the reference's tensor contract (float (B, 3k, H, W) device tensor in
        [0,255]); returns a new tensor (the reference paints the cover into its argument in place and returns a
        fresh noisy tensor).  ``colors`` / ``noise`` replace the random draws (tests)."""
        x = _device_batch(image_batch, self.input_shape)
        if colors is None:
            colors = self.draw_colors()
        if noise is None:
            noise = torch.randn(x.shape, device=x.device) * self.std
        out = torch.empty_like(x)
        ops.noisy_cover_nchw(x, noise.to(x.device, torch.float32).contiguous(), colors, self.top, self.bottom, out)
        return out


def make_augmentor(name, input_shape, output_shape=None, *, pad=4, min_cut=10, max_cut=30, conv_p=1.0, p=None,
                   degrees=10.0, scale=(0.9, 1.1), translate=0.05, fill='edge'):
    """augmentations.py:208-221, plus 'random_shift' (``pad``: its padding), 'cutout' / 'cutout_color' (``min_cut``,
    ``max_cut``: the range of a box side), 'random_conv' (``conv_p``: the probability that a sample is convolved),
    'translate' (``output_shape``: its canvas, None = 8 pixels more per side length) and 'flip' / 'rotate' / 'grayscale'
    (``p``: the probability that a sample is transformed, None = the class's default) and 'affine' (``degrees``, ``scale``,
    ``translate``, ``fill``: RandomAffine's ranges and border rule; ``p``: its probability, None = 1.0) -- all nine beyond
    the reference -- and '<move>+<paint>' with <move> one of 'random_crop', 'random_shift', 'translate' and <paint> one of 'cutout',
    'cutout_color': a ``Compose`` of the two, the paint built for the move's output_shape."""
    print(f'CHOSEN AUGMENTATION: {name}')
    if '+' in name:
        move, _, paint = name.partition('+')
        if move not in ('random_crop', 'random_shift', 'translate') or paint not in ('cutout', 'cutout_color'):
            raise ValueError('augmentation is not supported: %s' % name)
        move = (RandomCrop(input_shape, output_shape) if move == 'random_crop' else
                RandomShift(input_shape, pad) if move == 'random_shift' else RandomTranslate(input_shape, output_shape))
        return Compose(move, RandomCutout(move.output_shape, min_cut, max_cut, color=paint == 'cutout_color'))
    if name == 'identity':
        return IdentityAugmentation(input_shape)
    if name == 'random_crop':
        return RandomCrop(input_shape, output_shape)
    if name == 'color_jiggle':
        return ColorJiggle(input_shape)
    if name == 'noisy_cover':
        return NoisyCover(input_shape)
    if name == 'random_shift':
        return RandomShift(input_shape, pad)
    if name in ('cutout', 'cutout_color'):
        return RandomCutout(input_shape, min_cut, max_cut, color=name == 'cutout_color')
    if name == 'random_conv':
        return RandomConv(input_shape, conv_p)
    if name == 'translate':
        return RandomTranslate(input_shape, output_shape)
    if name in ('flip', 'rotate', 'grayscale'):
        cls = RandomFlip if name == 'flip' else RandomRotate if name == 'rotate' else RandomGrayscale
        return cls(input_shape) if p is None else cls(input_shape, p)
    if name == 'affine':
        return RandomAffine(input_shape, degrees, scale, translate, fill, 1.0 if p is None else p)
    raise ValueError('augmentation is not supported: %s' % name)
