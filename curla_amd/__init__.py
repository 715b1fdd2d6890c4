"""curla_amd: MI355X-native CURL + SAC learner (drop-in for the learner path of
paulvantieghem/curla: CurlSacAgent.update & friends, CNNEncoder/PixelEncoder,
ReplayBuffer, random_crop)."""
from .augmentations import ColorJiggle, Compose, IdentityAugmentation, NoisyCover, RandomAffine, RandomConv, RandomCrop, RandomCutout, RandomFlip, RandomGrayscale, RandomRotate, RandomShift, RandomTranslate, make_augmentor  # noqa: F401
from .curl_sac import Actor, Critic, CURL, CurlSacAgent, QFunction  # noqa: F401
from .encoder import CNNEncoder, PixelEncoder  # noqa: F401
from .utils import (FrameStack, ReplayBuffer, eval_mode, make_dir, module_hash, preprocess_obs,  # noqa: F401
                    set_seed_everywhere, soft_update_params)

__all__ = ["CurlSacAgent", "Actor", "Critic", "QFunction", "CURL", "CNNEncoder", "PixelEncoder", "ReplayBuffer",
           "RandomCrop", "RandomShift", "RandomCutout", "RandomTranslate", "RandomFlip", "RandomRotate", "RandomGrayscale", "RandomAffine", "Compose", "RandomConv", "IdentityAugmentation", "ColorJiggle", "NoisyCover", "make_augmentor", "eval_mode", "set_seed_everywhere",
           "soft_update_params", "FrameStack", "make_dir", "module_hash", "preprocess_obs"]
