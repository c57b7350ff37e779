"""Host logic of the SD1.5 PPO training driver (consolver_amd/train_ppo.py): the command line of run_ppo.sh, the batch sequence, the checkpoint lookup and
the prompt lookup.  No GPU."""
import argparse
import os

import pytest

from consolver_amd import train_ppo as tp

# the flags run_ppo.sh passes to train_ppo.py, with its values
RUN_PPO_SH = ["--pretrained_teacher_model=stable-diffusion-v1-5/stable-diffusion-v1-5", "--output_dir=outputs/depth_4order_cfg3_prod_num_action_11_1e-4",
              "--tracker_project_name=depth_4order_cfg3_prod_num_action_11_1e-4", "--enable_xformers_memory_efficient_attention", "--mixed_precision=fp16",
              "--resolution=512", "--learning_rate=1e-4", "--loss_type=huber", "--adam_weight_decay=1e-3", "--max_train_steps=3001",
              "--max_train_samples=4000000", "--dataloader_num_workers=16", "--validation_steps=100", "--checkpointing_steps=100",
              "--checkpoints_total_limit=20", "--train_batch_size=80", "--gradient_accumulation_steps=1", "--cfg=3", "--use_8bit_adam",
              "--resume_from_checkpoint=latest", "--report_to=wandb", "--seed=453645634", "--order_dim=4", "--scaler_dim=0", "--ppo_epochs=1",
              "--factor_embedding_dim=1024", "--factor_hidden_dim=256", "--factor_num_actions=11", "--reward_type=depth", "--ppo_type=discrete",
              "--gradient_checkpointing"]
OURS = ["--data_dir", "pairs", "--prompt-cache", "prompts.safetensors"]


def test_run_ppo_sh_command_line_parses_with_its_values():
    args, _ = tp.parse_args(RUN_PPO_SH + OURS)
    assert args.output_dir == "outputs/depth_4order_cfg3_prod_num_action_11_1e-4" and args.resolution == 512
    assert args.learning_rate == 1e-4 and args.adam_weight_decay == 1e-3 and args.max_train_steps == 3001
    assert args.checkpointing_steps == 100 and args.train_batch_size == 80 and args.cfg == 3.0 and args.seed == 453645634
    assert (args.order_dim, args.scaler_dim, args.ppo_epochs) == (4, 0, 1)
    assert (args.factor_embedding_dim, args.factor_hidden_dim, args.factor_num_actions) == (1024, 256, 11)
    assert args.reward_type == "depth" and args.resume_from_checkpoint == "latest" and args.ppo_type == "discrete"
    assert args.data_dir == "pairs" and args.prompt_cache == "prompts.safetensors" and not args.use_conv and not args.no_share and not args.no_group
    note = tp.ignored_note(args)
    for flag in tp.IGNORED:                         # run_ppo.sh passes every one of them
        assert flag in note, flag
    assert "fp32 AdamW" in note


def test_defaults_are_the_references():
    args, _ = tp.parse_args(OURS)
    assert (args.train_batch_size, args.ppo_epochs, args.order_dim, args.scaler_dim, args.reward_type) == (16, 4, 4, 2, "depth")
    assert (args.learning_rate, args.adam_beta1, args.adam_beta2, args.adam_weight_decay, args.adam_epsilon) == (1e-4, 0.9, 0.999, 1e-2, 1e-8)
    assert (args.max_grad_norm, args.clip_range, args.entropy_coef, args.cfg, args.checkpointing_steps) == (1.0, 0.2, 0.01, 3.0, 500)
    assert (args.factor_embedding_dim, args.factor_hidden_dim, args.factor_num_actions) == (4, 4, 4)
    assert args.max_train_steps is None and args.seed is None and args.resume_from_checkpoint is None and args.teacher_steps == 40
    assert tp.ignored_note(args) is None


@pytest.mark.parametrize("extra", [["--ppo_type", "continuous"], ["--gradient_accumulation_steps", "2"], ["--lr_scheduler", "cosine"]])
def test_refused_combinations_exit(extra, capsys):
    with pytest.raises(SystemExit):
        tp.parse_args(OURS + extra)
    assert extra[0] in capsys.readouterr().err


def test_missing_data_arguments_exit():
    with pytest.raises(SystemExit):
        tp.parse_args(["--data_dir", "pairs"])
    assert tp.parse_args(["--synthetic", "4"])[0].synthetic == 4


def test_resolution_must_be_the_vaes(capsys):
    ap = argparse.ArgumentParser()
    assert tp.check_resolution(ap, None, 64) == 512 and tp.check_resolution(ap, 512, 64) == 512 and tp.check_resolution(ap, 128, 16) == 128
    with pytest.raises(SystemExit):
        tp.check_resolution(ap, 512, 16)
    assert "--resolution 512" in capsys.readouterr().err


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("n_items,batch_size", [(40, 4), (37, 5), (3, 8)])
def test_batch_indices_tile_the_batch_sequence(world, n_items, batch_size):
    n_batches = -(-n_items // batch_size)
    seq = []
    for step in range(3 * n_batches):
        for rank in range(world):
            idx = tp.batch_indices(step, rank, world, n_items, batch_size)
            assert len(idx) == batch_size and all(0 <= j < n_items for j in idx)
            seq.append(idx)
    # the ranks of the steps, read in (step, rank) order, walk the batches of the unshuffled dataset in order, without overlap or gap
    for k, idx in enumerate(seq):
        b = k % n_batches
        assert idx == [(b * batch_size + j) % n_items for j in range(batch_size)], (k, idx)
    if n_items % batch_size and n_items > batch_size:
        last = seq[n_batches - 1]
        tail = n_items % batch_size
        assert last[:tail] == list(range(n_items - tail, n_items)) and last[tail:] == list(range(batch_size - tail))        # wraps round to the first items


def test_batch_indices_after_a_resume_is_the_step_that_would_have_come():
    # a pure function of the step: a run that stopped after 7 steps and resumes at global_step = 7 reads what the uninterrupted run reads at its 8th step
    whole = [tp.batch_indices(s, 1, 2, 37, 5) for s in range(12)]
    resumed = [tp.batch_indices(s, 1, 2, 37, 5) for s in range(7, 12)]
    assert resumed == whole[7:]
    assert whole[7] != whole[6]
    with pytest.raises(ValueError):
        tp.batch_indices(0, 2, 2, 37, 5)
    with pytest.raises(ValueError):
        tp.batch_indices(0, 0, 1, 0, 5)


def test_latest_checkpoint_ignores_malformed_names(tmp_path):
    assert tp.latest_checkpoint(str(tmp_path / "missing")) is None
    assert tp.latest_checkpoint(str(tmp_path)) is None
    for name in ("checkpoint-2", "checkpoint-10", "checkpoint-9", "checkpoint-", "checkpoint-abc", "checkpoint-11-old", "checkpoint", "checkpoints-50", "samples"):
        os.makedirs(tmp_path / name)
    (tmp_path / "checkpoint-99").write_text("a file, not a directory")
    assert tp.latest_checkpoint(str(tmp_path)) == "checkpoint-10"


def test_prompt_lookup_raises_on_a_missing_prompt():
    index = {"a cat": 0, "a dog": 1}
    assert tp.prompt_rows(index, ["a dog", "a cat ", "a dog"]) == [1, 0, 1]
    with pytest.raises(KeyError, match="a horse"):
        tp.prompt_rows(index, ["a cat", "a horse"])


def test_param_sum_comparison():
    assert tp.check_param_sums([1.5]) == 1.5 and tp.check_param_sums([2.0, 2.0, 2.0]) == 2.0
    with pytest.raises(RuntimeError, match="diverged"):
        tp.check_param_sums([2.0, 2.0000001])
