"""Small helpers of the learner path (reference: utils.py).  The reference's module also holds the replay buffer:
``ReplayBuffer`` lives in replay.py (its write side in replay_write.py, its read side in replay_sample.py) and is
re-exported here, so ``utils.ReplayBuffer`` resolves as it does there."""
import collections
import os
import random

import numpy as np
import torch

from . import ops
from .replay import PerHandle, ReplayBuffer  # noqa: F401


class eval_mode(object):
    """Context manager that puts the given models (anything with ``.training`` and ``.train(bool)``) in
    evaluation mode and restores each one's previous mode on exit (utils.py:21-34)."""

    def __init__(self, *models):
        self.models = models
        self._was_training = None

    def __enter__(self):
        self._was_training = [m.training for m in self.models]
        for m in self.models:
            m.train(False)

    def __exit__(self, *exc):
        for m, mode in zip(self.models, self._was_training):
            m.train(mode)
        return False


def soft_update_params(net, target_net, tau):
    """utils.py:37-41, one fused lerp kernel per tensor.  CurlSacAgent uses the
    flat-buffer form (``soft_update_targets``): two launches for all 24 tensors."""
    for param, target_param in zip(net.parameters(), target_net.parameters()):
        ops.soft_update(param.data.view(-1), target_param.data.view(-1), tau)


def set_seed_everywhere(seed):
    """utils.py:44-49."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def make_dir(dir_path):
    """Create ``dir_path`` unless it exists; like the reference (utils.py:61-66) a failure is reported, not raised,
    and the path is returned either way."""
    if not os.path.isdir(dir_path):
        try:
            os.mkdir(dir_path)
        except OSError as e:
            print('Unable to create directory %s (%s)' % (dir_path, e.strerror))
    return dir_path


def module_hash(module):
    """Sum of the sums of a module's state_dict tensors -- the reference's cheap "did the weights change" number
    (utils.py:50-54)."""
    return sum(t.sum().item() for t in module.state_dict().values())


def preprocess_obs(obs, bits=5):
    """Bit-depth reduction with uniform dequantisation noise, arXiv:1807.03039 (utils.py:67-77; unused by the
    learner path, kept so that ``utils.`` resolves every name the reference module has)."""
    assert obs.dtype == torch.float32
    bins = 2 ** bits
    if bits < 8:
        obs = torch.floor(obs / 2 ** (8 - bits))
    return obs / bins + torch.rand_like(obs) / bins - 0.5


class FrameStack(object):
    """Observation wrapper that returns the last ``k`` frames concatenated on the channel axis (utils.py:238-268):
    ``reset`` fills the stack with k copies of the first frame, ``step`` pushes the new frame.  Plain duck-typed
    wrapper (``gymnasium`` is only used for the observation space when it is importable): every other attribute
    is forwarded to the wrapped environment, as ``gym.Wrapper`` does."""

    def __init__(self, env, k):
        self.env = env
        self._k = k
        self._frames = collections.deque([], maxlen=k)
        space = getattr(env, "observation_space", None)
        shp = tuple(getattr(space, "shape", ()))
        if shp:
            stacked = (shp[0] * k,) + shp[1:]
            try:
                import gymnasium
                self.observation_space = gymnasium.spaces.Box(low=0, high=1, shape=stacked, dtype=space.dtype)
            except ImportError:
                self.observation_space = type("Box", (), dict(shape=stacked, dtype=getattr(space, "dtype", np.uint8),
                                                              low=0, high=1))()
        self._max_episode_steps = getattr(env, "_max_episode_steps", None)
        self.curl_driving = False

    def __getattr__(self, name):  # only called for attributes not found on the wrapper itself
        if name in ("env", "_frames"):
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self):
        first = self.env.reset()
        self.curl_driving = getattr(self.env, "curl_driving", False)
        self._frames.extend([first] * self._k)
        return self._get_obs()

    def step(self, action):
        frame, reward, done, info = self.env.step(action)
        self.env.curl_driving = self.curl_driving
        self._frames.append(frame)
        return self._get_obs(), reward, done, info

    def _get_obs(self):
        assert len(self._frames) == self._k
        return np.concatenate(list(self._frames), axis=0)

