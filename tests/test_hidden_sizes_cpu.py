"""The hidden sizes (--rnn-out) the GPU fast paths take: model.hidden_size_support, the one predicate behind new_cache,
Agent.loss_recompute's choice of the fused heads, boot_values and the action draw; and the refusal of a size without a draw."""
import pytest
import torch

from active_tracking_rl_amd import model as M

# R: (rollout cache + cell kernels, fused heads + loss, fused action draw, bootstrap value through the rollout's kernels)
TABLE = {32: (True, False, True, False), 64: (True, True, True, True), 96: (True, False, True, False),
         128: (True, True, True, True), 130: (False, False, False, False), 192: (True, False, True, False),
         256: (True, True, True, False), 512: (True, False, False, False)}


@pytest.mark.parametrize("R", sorted(TABLE))
def test_hidden_size_support_table(R):
    s = M.hidden_size_support(R)
    assert (s["cache"], s["fused_heads"], s["fused_sampler"], s["fused_boot"]) == TABLE[R]
    assert set(s) == {"cache", "fused_heads", "fused_sampler", "fused_boot"}
    # what the kernels themselves accept (csrc/heads_hip.hip: R / 4 lanes per row; csrc/policy_hip.hip: kMaxR; the cells: R % 4)
    assert s["fused_heads"] == (R % 4 == 0 and R // 4 in (16, 32, 64))
    assert s["fused_sampler"] == (R % 4 == 0 and R <= 256)
    if s["fused_heads"]:
        assert s["cache"] and s["fused_sampler"]
    # (the bootstrap step needs the critic-head kernel; R = 256 has it and still takes the model's own forward: model.BOOT_MAX_R)
    assert s["fused_boot"] == (s["fused_heads"] and R <= 128)


@pytest.mark.parametrize("R", sorted(TABLE))
def test_a_size_without_a_draw_is_refused_for_the_gpu_only(R):
    M.check_hidden_size(R, torch.device("cpu"))
    M.check_hidden_size(R, None)
    if TABLE[R][2]:
        M.check_hidden_size(R, torch.device("cuda:0"))
        M.check_hidden_size(R, "cuda")
    else:
        with pytest.raises(ValueError, match="multiples of 4 up to 256") as e:
            M.check_hidden_size(R, torch.device("cuda:0"))
        assert "--rnn-out %d" % R in str(e.value) and "64, 128, 256" in str(e.value)

