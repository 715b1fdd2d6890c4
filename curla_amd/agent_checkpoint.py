"""CurlSacAgent on disk: the reference's three state_dict files (save / load) and the full training state
(save_checkpoint / load_checkpoint) -- the reference only writes the former and cannot resume; the latter adds log_alpha,
the target critic, the five Adam states, the RNG streams, the step and what each option's mixin keeps (its
``_x_checkpoint()`` / ``_load_x_checkpoint(ck)`` pair)."""
import warnings

import numpy as np
import torch

# settings a file carries for the warning alone -- the agent keeps its own: (name, as saved, a file from before the
# keyword, saved at that value too)
_WARN_ONLY = (("critic_dropout", float, 0.0, True), ("utd_ratio", int, 1, True), ("aug_views", int, 1, False))


class _CheckpointMixin:
    """CurlSacAgent's save / load methods."""

    def save(self, model_dir, augmentation, step):
        """curl_sac.py:453-456 (same three files, reference tensor layouts)."""
        torch.save(self.CURL.state_dict(), '%s/%s_curl_%s.pt' % (model_dir, augmentation, step))
        torch.save(self.actor.state_dict(), '%s/%s_actor_%s.pt' % (model_dir, augmentation, step))
        torch.save(self.critic.state_dict(), '%s/%s_critic_%s.pt' % (model_dir, augmentation, step))

    def load(self, model_dir, augmentation, step):
        """curl_sac.py:458-465 (same files, same three progress lines on stdout)."""
        curl = torch.load('%s/%s_curl_%s.pt' % (model_dir, augmentation, step))
        self._check_curl_state_dict(curl)  # (the other objective's file: refused before anything is written)
        self.CURL.load_state_dict(curl)
        print('Loaded model %s/%s_curl_%s.pt' % (model_dir, augmentation, step))
        self.actor.load_state_dict(torch.load('%s/%s_actor_%s.pt' % (model_dir, augmentation, step)))
        print('Loaded model %s/%s_actor_%s.pt' % (model_dir, augmentation, step))
        self.critic.load_state_dict(torch.load('%s/%s_critic_%s.pt' % (model_dir, augmentation, step)))
        self.critic_target.load_state_dict(self.critic.state_dict())
        print('Loaded model %s/%s_critic_%s.pt' % (model_dir, augmentation, step))

    def save_checkpoint(self, path, step):
        rng = {"torch": torch.get_rng_state(), "numpy": np.random.get_state()}
        if self.device.type == "cuda":
            rng["cuda"] = torch.cuda.get_rng_state(self.device)
        torch.save({
            "format": "curla_amd.checkpoint.v1", "step": int(step),
            "actor": self.actor.state_dict(), "critic": self.critic.state_dict(),
            "critic_target": self.critic_target.state_dict(), "curl": self.CURL.state_dict(),
            "log_alpha": self.log_alpha.detach().cpu(),
            "optimizers": {k: self._convert_opt_state(o, o.state_dict(), True) for k, o in self._optimizers().items()},
            "rng": rng,
            **{name: cast(getattr(self, name)) for name, cast, default, always in _WARN_ONLY
               if always or getattr(self, name) != default},
            **self._critic_head_checkpoint(), **self._policy_checkpoint(), **self._reset_checkpoint(),
            **self._redo_checkpoint(), **self._cpc_checkpoint(),
        }, path)

    def load_checkpoint(self, path, restore_rng=True):
        """Returns the step the checkpoint was written at."""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if ck.get("format") != "curla_amd.checkpoint.v1":
            raise ValueError("not a curla_amd checkpoint: %r" % (path,))
        self._check_cpc_checkpoint(ck)  # (the other objective's file: refused before anything is written)
        for name, _, default, _ in _WARN_ONLY:
            if ck.get(name, default) != getattr(self, name):
                warnings.warn("curla_amd: the checkpoint was written with %s = %r; this agent keeps its own, %r"
                              % (name, ck.get(name, default), getattr(self, name)), RuntimeWarning, stacklevel=2)
        self.CURL.load_state_dict(ck["curl"])
        self.actor.load_state_dict(ck["actor"])
        self.critic.load_state_dict(ck["critic"])
        self.critic_target.load_state_dict(ck["critic_target"])
        self._load_critic_head_checkpoint(ck)
        self._load_policy_checkpoint(ck)
        with torch.no_grad():
            self.log_alpha.copy_(ck["log_alpha"])
        for k, o in self._optimizers().items():
            o.load_state_dict(self._convert_opt_state(o, ck["optimizers"][k], False))
        if restore_rng:
            torch.set_rng_state(ck["rng"]["torch"])
            np.random.set_state(ck["rng"]["numpy"])
            if self.device.type == "cuda" and "cuda" in ck["rng"]:
                torch.cuda.set_rng_state(ck["rng"]["cuda"], self.device)
        self._load_reset_checkpoint(ck)
        self._load_redo_checkpoint(ck)
        self._drop_encoder_caches()
        # captured graphs hold the addresses of log_alpha's Adam moments, which load_state_dict has just replaced
        self._drop_graphs()
        return ck["step"]
