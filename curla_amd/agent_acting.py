"""Acting with CurlSacAgent: one observation (the reference's select_action / sample_action) or a batch of them."""
import numpy as np
import torch

from . import ops
from .augmentations import Compose, RandomCrop, RandomTranslate


class _ActingMixin:
    """CurlSacAgent's acting methods; the state they use (``_act_stage``, ``_act_batch_stage``) is the agent's."""

    def _stage_obs(self, obs):
        """One observation for the actor.  uint8 (C, H, W) frames -- what the environment and train.py hand over --
        go through a pinned host buffer into a one-slot uint8 NHWC device ring and are read by the same fused
        conv1 loader as a replay minibatch (52 KB over PCIe instead of a pageable 208 KB float copy); anything else
        takes the reference's torch.FloatTensor(obs) route (curl_sac.py:332-333)."""
        if not (isinstance(obs, np.ndarray) and obs.dtype == np.uint8 and obs.ndim == 3):
            return torch.FloatTensor(np.ascontiguousarray(obs)).to(self.device).unsqueeze(0)
        C, H, W = obs.shape
        st = self._act_stage.get((C, H, W))
        if st is None:
            n = H * W * C
            pin = torch.empty(n, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
            ring = torch.zeros(n + 32, dtype=torch.uint8, device=self.device)  # + loader slack (curla_hip.h)
            st = self._act_stage[(C, H, W)] = (pin, pin.numpy().reshape(H, W, C), ring, ring[:n].view(1, H, W, C))
        pin, pin_hwc, ring, frames = st
        np.copyto(pin_hwc, obs.transpose(1, 2, 0))
        ring[:pin.numel()].copy_(pin, non_blocking=True)
        return ops.ObsRef.from_ring(frames, None, None, None, 1, (H, W))

    def select_action(self, obs):
        """curl_sac.py:330-337."""
        with torch.no_grad():
            mu, _, _, _ = self.actor(self._stage_obs(obs), compute_pi=False, compute_log_pi=False)
            return mu.cpu().data.numpy().flatten()

    def sample_action(self, obs, noise=None):
        """curl_sac.py:339-347."""
        if obs.shape[-2:] != self.image_shape:
            obs = self.augmentor.evaluation_augmentation(obs)
        with torch.no_grad():
            mu, pi, _, _ = self.actor(self._stage_obs(obs), compute_log_pi=False, noise=noise)
            return pi.cpu().data.numpy().flatten()

    # ------------------------------------------------------------------ acting on a batch of observations
    _ACT_PINS = 2  # pinned host blocks per frame shape, used in rotation

    def _act_windows(self):
        """Frame sizes the batched acting calls take -> origin of the window the encoder reads: its own size (the
        whole frame) and, under a RandomCrop, the crop's input size (the centre window of
        RandomCrop.evaluation_augmentation, augmentations.py:26-45).  Under a RandomTranslate also the translate's input
        size, with None for an origin: such frames are no window of anything, they are centred on a black canvas as
        RandomTranslate.evaluation_augmentation does (_act_centred), whatever the margins (0 and 1 included).  A Compose
        acts as its ``move`` does: the cutout's evaluation is the identity."""
        h, w = self.image_shape
        windows = {(h, w): (0, 0)}
        aug = self.augmentor
        if isinstance(aug, Compose):
            aug = aug.move
        if isinstance(aug, (RandomCrop, RandomTranslate)) and tuple(aug.output_shape) == (h, w):
            H, W = aug.input_shape
            windows.setdefault((H, W), ((H - h) // 2, (W - w) // 2) if isinstance(aug, RandomCrop) else None)
        return windows

    def _act_centred(self, x, shape):
        """(RandomTranslate) N frames of the translate's input size, each centred on a zero canvas of the encoder's size
        exactly as ``evaluation_augmentation`` centres one: host arrays with NumPy, tensors with torch where they are.
        Not a hot path: acting on frames of the encoder's own size stages them as before."""
        N, C, H, W = shape
        h, w = self.image_shape
        top, left = (h - H) // 2, (w - W) // 2
        if torch.is_tensor(x):
            out = torch.zeros((N, C, h, w), dtype=x.dtype, device=x.device)
        else:
            x = np.stack(x) if isinstance(x, list) else x
            out = np.zeros((N, C, h, w), dtype=x.dtype)
        out[:, :, top:top + H, left:left + W] = x
        return out, (N, C, h, w), (0, 0)

    def _act_batch_args(self, obs, noise):
        """Argument checks of select_actions / sample_actions (they come before anything touches the device).
        Returns (x, (N, C, H, W), (top, left)); ``x`` is ``obs``, a list of uint8 frames, or a stacked array."""
        C, A = self.actor.encoder.obs_shape[0], self.action_dim
        windows = self._act_windows()
        want = "expected (N, %d, H, W) with N >= 1 and (H, W) = %s" % (C, " or ".join(str(s) for s in windows))
        x = obs
        if torch.is_tensor(obs) or isinstance(obs, np.ndarray):
            shape = tuple(obs.shape)
        else:
            x = list(obs)
            if not x:
                raise ValueError("empty batch of observations: " + want)
            shape = (len(x),) + tuple(np.shape(x[0]))
            if any(tuple(np.shape(f)) != shape[1:] for f in x):
                raise ValueError("observations of different shapes in one batch: " + want)
            if not all(isinstance(f, np.ndarray) and f.dtype == np.uint8 for f in x):
                x = np.stack([np.asarray(f.cpu() if torch.is_tensor(f) else f) for f in x])
        if len(shape) != 4 or shape[0] < 1 or shape[1] != C or shape[2:] not in windows:
            raise ValueError("observation batch of shape %s: %s" % (shape, want))
        if noise is not None and not (torch.is_tensor(noise) and tuple(noise.shape) == (shape[0], A)):
            raise ValueError("noise of shape %s: expected an (N, A) = (%d, %d) tensor"
                             % (tuple(getattr(noise, "shape", ())), shape[0], A))
        from . import _lib
        if self.device.type != "cuda" and _lib._trace_hook is None:
            raise RuntimeError("CurlSacAgent.select_actions / sample_actions need a CUDA/HIP device: the acting path "
                               "has no CPU fallback")
        window = windows[shape[2:]]
        if window is None:
            return self._act_centred(x, shape)
        return x, shape, window

    def _stage_obs_batch(self, x, shape, window):
        """N observations for the actor.  uint8 frames go planar, as they are, into a pinned block (one contiguous
        host copy), over PCIe in one asynchronous copy, and through ONE ops.stage_frames launch -- transpose and
        centre window fused -- into N slots of a uint8 NHWC device ring that the first conv's loader reads like a
        replay minibatch; a uint8 CUDA tensor skips the host part.  Anything else takes the reference's
        torch.FloatTensor route (curl_sac.py:332-333) as a batch.  Blocks and ring are kept per (C, H, W), sized for
        the largest N seen; a pinned block is written again only after its copy has executed (an event per block)."""
        N, C, H, W = shape
        top, left = window
        h, w = self.image_shape
        if torch.is_tensor(x) and x.dtype == torch.uint8 and not x.is_cuda:
            x = x.numpy()
        on_device = torch.is_tensor(x) and x.dtype == torch.uint8
        if not (on_device or isinstance(x, list) or (isinstance(x, np.ndarray) and x.dtype == np.uint8)):
            if torch.is_tensor(x):
                return x[:, :, top:top + h, left:left + w].to(self.device, torch.float32).contiguous()
            return torch.FloatTensor(np.ascontiguousarray(x[:, :, top:top + h, left:left + w])).to(self.device)
        cuda = self.device.type == "cuda"
        st = self._act_batch_stage.get((C, H, W))
        if st is None or st["cap"] < N:
            ring = torch.zeros(N * h * w * C + 32, dtype=torch.uint8, device=self.device)  # + loader slack (curla_hip.h)
            st = self._act_batch_stage[(C, H, W)] = dict(cap=N, ring=ring, src=None, pins=None, turn=0)
        n_src = N * C * H * W
        if on_device:
            src = x.to(self.device).contiguous()
        else:
            if st["src"] is None:
                cap = st["cap"] * C * H * W
                st["src"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
                pins = [torch.empty(cap, dtype=torch.uint8, pin_memory=cuda) for _ in range(self._ACT_PINS)]
                st["pins"] = [(p, p.numpy(), torch.cuda.Event() if cuda else None) for p in pins]
            k = st["turn"]
            st["turn"] = (k + 1) % len(st["pins"])
            pin, pin_np, event = st["pins"][k]
            if cuda:
                event.synchronize()  # (returns at once unless the copy out of this block is still to run)
            host = pin_np[:n_src].reshape(N, C, H, W)
            if isinstance(x, list):
                np.stack(x, out=host)
            else:
                np.copyto(host, x)
            src = st["src"][:n_src].view(N, C, H, W)
            src.copy_(pin[:n_src].view(N, C, H, W), non_blocking=True)
            if cuda:
                event.record()
        frames = st["ring"][:N * h * w * C].view(N, h, w, C)
        ops.stage_frames(src, frames, 0, top, left)
        return ops.ObsRef.from_ring(frames, None, None, None, N, (h, w))

    def select_actions(self, obs, as_tensor=False):
        """``select_action`` (curl_sac.py:330-337) row by row for N observations in one pass: the (N, A) float32
        means.  ``obs``: a uint8 array (N, C, H, W), a sequence of N uint8 (C, H, W) frames or a uint8 CUDA tensor
        (the fast route, _stage_obs_batch); anything else (float arrays) goes the reference's float route.  (H, W) is
        the encoder's input size or -- under a RandomCrop -- the crop's input size, whose centre window is then cut
        inside the staging launch, or -- under a RandomTranslate -- the translate's input size, which is then centred on
        a black canvas like ``evaluation_augmentation`` does; any other size raises ValueError.  Returns a NumPy array (one device -> host
        copy, one synchronisation), or with ``as_tensor`` the device tensor without synchronising; that tensor is
        storage of its own, which later acting calls do not touch.  Builds no autograd graph, draws no random
        numbers, and leaves the update's workspaces, index blocks and captured graphs alone."""
        x, shape, window = self._act_batch_args(obs, None)
        with torch.no_grad():
            mu, _, _, _ = self.actor(self._stage_obs_batch(x, shape, window), compute_pi=False, compute_log_pi=False)
        return mu if as_tensor else mu.cpu().numpy()

    def sample_actions(self, obs, noise=None, as_tensor=False):
        """``sample_action`` (curl_sac.py:339-347) row by row for N observations in one pass: the (N, A) float32
        samples.  ``obs``, the accepted sizes and the return value as in ``select_actions``.  ``noise`` (N, A)
        replaces the draw; without it the draw is Actor.forward's single ``torch.randn((N, A), device=...)``, so a
        seeded call equals the call with that tensor passed in."""
        x, shape, window = self._act_batch_args(obs, noise)
        if noise is not None:
            noise = noise.detach().to(self.device, torch.float32).contiguous()
        with torch.no_grad():
            _, pi, _, _ = self.actor(self._stage_obs_batch(x, shape, window), compute_log_pi=False, noise=noise)
        return pi if as_tensor else pi.cpu().numpy()
