"""The checkpoint format ``curla_amd.checkpoint.v1`` key for key: what ``save_checkpoint`` writes for an agent with every
option off and with one option on, on CPU agents at the ``b8`` shape of tests/test_update_launches_host.py.  The key sets
are literals, written down from the files of the commit before the options' checkpoint entries moved into their mixins'
``_x_checkpoint()`` / ``_load_x_checkpoint(ck)`` pairs (agent_checkpoint.py)."""
import warnings

import pytest
import torch

from tests.test_update_launches_host import make

CORE = {"format", "step", "actor", "critic", "critic_target", "curl", "log_alpha", "optimizers", "rng", "critic_dropout",
        "utd_ratio", "critic_quantiles", "critic_drop_quantiles", "reset_rng", "reset_epoch", "reset_count",
        "reset_interval", "reset_encoder_keep", "reset_seed"}
# case -> (the description ``make`` takes, the keys beside CORE, the values of the scalar entries that tell the option)
CONFIGS = {
    "off": ({}, set(), dict(critic_dropout=0.0, utd_ratio=1, critic_quantiles=0, critic_drop_quantiles=0)),
    "bins": (dict(agent=dict(critic_bins=5, critic_value_range=(-4.0, 6.0))),
             {"critic_bins", "critic_value_range", "critic_bin_sigma"},
             dict(critic_bins=5, critic_value_range=(-4.0, 6.0), critic_bin_sigma=0.75, critic_quantiles=0)),
    "quantiles": (dict(agent=dict(critic_quantiles=5, critic_drop_quantiles=1)), set(),
                  dict(critic_quantiles=5, critic_drop_quantiles=1)),
    "deterministic": (dict(agent=dict(policy="deterministic")),
                      {"policy", "policy_std", "policy_std_clip", "policy_std_schedule"},
                      dict(policy="deterministic", policy_std=0.2, policy_std_clip=0.3, policy_std_schedule=None)),
    "aug_views": (dict(agent=dict(aug_views=2), rb=dict(aug_views=2)), {"aug_views"}, dict(aug_views=2)),
}


@pytest.mark.parametrize("case", sorted(CONFIGS))
def test_save_checkpoint_writes_exactly_these_keys(case, tmp_path):
    spec, extra, values = CONFIGS[case]
    agent, _ = make(spec)
    path = str(tmp_path / "ck.pt")
    agent.save_checkpoint(path, 3)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == CORE | extra
    assert ck["format"] == "curla_amd.checkpoint.v1" and ck["step"] == 3
    for k, v in values.items():
        assert ck[k] == v and type(ck[k]) is type(v), k
    assert set(ck["optimizers"]) == {"actor", "critic", "log_alpha", "encoder", "cpc"}
    assert set(ck["rng"]) == {"torch", "numpy"}
    # ... and a second agent of the same kind takes the file without a warning
    other, _ = make(spec, seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert other.load_checkpoint(path) == 3
    for k, v in agent.critic.state_dict().items():
        assert torch.equal(v, other.critic.state_dict()[k]), k


def test_the_three_saved_settings_warn_with_their_texts(tmp_path):
    path = str(tmp_path / "ck.pt")
    make(dict(agent=dict(critic_layer_norm=True, critic_dropout=0.1, utd_ratio=2)))[0].save_checkpoint(path, 1)
    other, _ = make(dict(agent=dict(critic_layer_norm=True, aug_views=2), rb=dict(aug_views=2)))
    with pytest.warns(RuntimeWarning) as seen:
        other.load_checkpoint(path)
    assert [str(w.message) for w in seen] == [
        "curla_amd: the checkpoint was written with critic_dropout = 0.1; this agent keeps its own, 0.0",
        "curla_amd: the checkpoint was written with utd_ratio = 2; this agent keeps its own, 1",
        "curla_amd: the checkpoint was written with aug_views = 1; this agent keeps its own, 2"]
    assert (other.critic_dropout, other.utd_ratio, other.aug_views) == (0.0, 1, 2)
