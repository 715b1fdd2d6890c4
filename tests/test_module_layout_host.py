"""The learner's modules after the split of curl_sac.py by subject: every name the one-file
curl_sac defined is still importable from it, no method or class attribute was lost on the way, and the MLP launch
helpers and autograd stand below curl_sac in the import order."""
import os
import subprocess
import sys

import pytest

import curla_amd.curl_sac as curl_sac

PACKAGE = os.path.dirname(os.path.abspath(curl_sac.__file__))

# name -> the module that holds it now; the list is the one-file curl_sac's own namespace
MOVED = {
    "mlp": ["_Mlp", "_MlpLn", "_linears", "_mlp_fwd", "_mlp_bwd"],
    "networks": ["Actor", "QFunction", "Critic", "CURL", "weight_init", "LOG_FREQ", "_QFunctionType", "_CriticType",
                 "_widen_last_layers", "_check_quantiles", "_check_drop_quantiles", "_check_layer_norm_width",
                 "_check_dropout", "_device_generator", "_reserve_dropout_counter", "_check_int", "_check_bins",
                 "_check_value_range", "_check_bin_sigma", "_check_policy_std", "_check_policy_std_clip"],
    "agent_graphs": ["_NullLog", "_UpdateGraphsMixin"],
    "agent_policy": ["_check_policy", "_check_policy_std_schedule", "_linear_schedule", "_policy_keywords", "_PolicyMixin"],
    "agent_critic_head": ["_critic_head_keywords", "_CriticHeadMixin"],
    "agent_optim": ["_OptimMixin"],
    "agent_checkpoint": ["_CheckpointMixin"],
    "agent_reset": ["_check_reset_interval", "_check_reset_keep", "_check_reset_seed", "_reset_keywords", "_ResetMixin"],
    "agent_redo": ["_check_redo_interval", "_check_redo_tau", "_check_redo_recycle", "_redo_keywords", "_RedoMixin"],
}
KEPT = ["CurlSacAgent", "_AgentType", "_Workspace", "_as_ref", "_check_utd_ratio", "_no_drop", "CNNEncoder", "ObsRef",
        "FlatAdam", "check_max_grad_norm", "check_weight_decay", "_check_views"]


def test_every_name_of_the_one_file_module_is_importable_from_curl_sac_and_is_its_new_homes_object():
    import importlib
    for module, names in MOVED.items():
        home = importlib.import_module("curla_amd." + module)
        for name in names:
            assert getattr(curl_sac, name) is getattr(home, name), (module, name)
    for name in KEPT:
        assert hasattr(curl_sac, name), name


# dir() of the classes before the split, dunders removed: what torch.nn.Module brought, then each class's own
MODULE = """T_destination _apply _call_impl _compiled_call_impl _get_backward_hooks _get_backward_pre_hooks _get_name
    _load_from_state_dict _maybe_warn_non_full_backward_hook _named_members _register_load_state_dict_pre_hook
    _register_state_dict_hook _replicate_for_data_parallel _save_to_state_dict _slow_forward _version
    _wrapped_call_impl add_module apply bfloat16 buffers call_super_init children compile cpu cuda double
    dump_patches eval extra_repr float forward get_buffer get_extra_state get_parameter get_submodule half ipu
    load_state_dict modules mtia named_buffers named_children named_modules named_parameters parameters
    register_backward_hook register_buffer register_forward_hook register_forward_pre_hook
    register_full_backward_hook register_full_backward_pre_hook register_load_state_dict_post_hook
    register_load_state_dict_pre_hook register_module register_parameter register_state_dict_post_hook
    register_state_dict_pre_hook requires_grad_ set_extra_state set_submodule share_memory state_dict to to_empty
    train type xpu zero_grad""".split()
ATTRIBUTES = {
    "CurlSacAgent": """GRAPH_CAPTURE_RETRIES _ACT_PINS _act_batch_args _act_centred _act_windows _actor_norm_log
        _actor_step_pending _actor_steps _allreduce _allreduce_wait _check_n_step _clip_torch _convert_opt_state
        _curl_unfused _defer_actor_step _drop_graphs _dropout _encoder_backward _finish_actor_step _grad_offset
        _graph_capture_agreed _graph_key _graph_kind _graph_live _graph_rb_key _graph_tail _graph_usable
        _graphed_substep _install_grad_views _leading_phases _max_grad_norm _noise _noise_launch _optimizers _records
        _replica_checksum _restore_grad_views _soft_update_done _soft_update_hint _stage_obs _stage_obs_batch
        _substep_eager _takes_want_pos _to_flat_device_layout _update_eager _update_graphed _update_phases
        _utd_leading _want_pos_known _ws alpha check_replicas critic_drop_quantiles critic_dropout critic_layer_norm
        critic_quantiles disable_update_graphs enable_data_parallel enable_update_graphs grad_clip_stats load
        load_checkpoint max_grad_norm sample_action sample_actions save save_checkpoint select_action select_actions
        set_max_grad_norm set_weight_decay soft_update_targets train update update_actor_and_alpha update_cpc
        update_critic utd_ratio weight_decay
        _actor_fwd _actor_kw _actor_loss _actor_out_dim _actor_reduce_and_step _anchor_cache _check_aug_views _cpc_steps
        _critic_forward _critic_loss _critic_step _critic_width_kw _draw_fresh _drop_encoder_caches
        _encoder_backward_reduced _hlg_last_B _hlg_params _load_redo_checkpoint _load_reset_checkpoint _maybe_reset
        _next_policy _online_q _phases _policy_clip _policy_std _pos_cache _pos_fc_done _pos_hint _q_four _q_merged
        _q_unmerged _redo_allreduce _redo_buf _redo_buffers _redo_checkpoint _redo_due _redo_moments _redo_pass
        _redo_scheduled _replica_check_due _reset_checkpoint _reset_epoch _reset_handover _reset_rng _reset_stage
        _reset_staging _reset_stream _stage_fresh _stage_params _target_q _twin_bwd _twin_fwd _upload_fresh aug_views
        critic_bin_sigma critic_bins critic_value_range dormant_counts dormant_fractions dormant_report policy policy_std
        policy_std_clip policy_std_schedule redo_count redo_interval redo_pass redo_recycle redo_tau reset_count
        reset_encoder_keep reset_interval reset_networks reset_seed set_policy_std target_clip_fraction""".split(),
    "Actor": MODULE + ["log"],
    "Critic": MODULE + ["DROP_TAG_FORWARD", "dropout", "log", "out_dim", "quantiles", "twin", "twin_ln"],
    "QFunction": MODULE + ["quantiles"],
    "CURL": MODULE + ["compute_logits", "encode"],
}


@pytest.mark.parametrize("cls", sorted(ATTRIBUTES))
def test_no_attribute_of_a_class_was_lost_in_the_move(cls):
    have = set(dir(getattr(curl_sac, cls)))
    assert len(ATTRIBUTES[cls]) == len(set(ATTRIBUTES[cls])) >= 70
    assert [a for a in ATTRIBUTES[cls] if a not in have] == []


# ``import curla_amd.mlp`` runs the package's __init__ first, which imports curl_sac for the public names and stays as
# it is: the child stands a bare package object in for it, so that what it observes is the two modules' own imports.
CHILD = """import sys, types
package = types.ModuleType("curla_amd")
package.__path__ = [sys.argv[1]]
sys.modules["curla_amd"] = package
import curla_amd.mlp
import curla_amd.autograd
import curla_amd.agent_critic_head
import curla_amd.agent_policy
import curla_amd.agent_optim
import curla_amd.agent_checkpoint
sys.exit(3 if "curla_amd.curl_sac" in sys.modules else 0)
"""


def test_mlp_and_autograd_import_without_curl_sac():
    for module in ("mlp.py", "autograd.py", "agent_critic_head.py", "agent_policy.py", "agent_optim.py",
                   "agent_checkpoint.py"):
        with open(os.path.join(PACKAGE, module)) as f:
            assert "curl_sac import" not in f.read(), module
    child = subprocess.run([sys.executable, "-c", CHILD, PACKAGE], capture_output=True, text=True)
    assert child.returncode == 0, (child.returncode, child.stderr[-2000:])
