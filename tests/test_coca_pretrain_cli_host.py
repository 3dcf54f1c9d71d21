"""coca_pretrain.py without a GPU: its flags and defaults are the reference's (coca_pretrain.py:27-67, written out here), plus
--max_steps and --num_workers; with no GPU visible it ends with the message the other HIP-only command lines give."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["data_dir", "output_dir", "model_name", "config_file", "pretrained_text_model_path", "pretrained_image_model_path"]
# flag -> (default, type) as the reference declares them
REFERENCE = {
    "seed": (2345, int), "train_batch_size": (64, int), "learning_rate": (1e-3, float), "start_epoch": (0, int),
    "num_train_epochs": (1000, int), "weight_decay": (1e-5, float), "log_steps": (None, int), "file_state_dict": (None, str),
    "parameters_to_freeze": (None, str), "warmup_proportion": (0.1, float), "gradient_accumulation_steps": (1, int),
    "adam_epsilon": (1e-8, float), "fp16": (False, None), "image_model_name": ("vit_base_patch16_384", str), "image_size": (384, int),
    "hflip": (0.5, float), "color_jitter": (None, float), "do_lower_case": (True, bool), "max_seq_len": (None, int),
    "max_seq_len_pv": (None, int), "caption_loss_weight": (1.0, float), "contrastive_loss_weight": (1.0, float),
}
ADDED = {"max_steps": (-1, int), "num_workers": (0, int)}


def load_script():
    spec = importlib.util.spec_from_file_location("coca_pretrain_cli", os.path.join(ROOT, "coca_pretrain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_and_defaults_are_the_reference_s():
    parser = load_script().get_parser()
    actions = {a.dest: a for a in parser._actions if a.dest != "help"}
    assert sorted(actions) == sorted(REQUIRED + list(REFERENCE) + list(ADDED))
    for name in REQUIRED:
        assert actions[name].required and actions[name].type is str, name
    for name, (default, kind) in {**REFERENCE, **ADDED}.items():
        a = actions[name]
        assert not a.required and a.default == default and type(a.default) is type(default), (name, a.default)
        if kind is None:
            assert a.nargs == 0 and a.const is True, name           # store_true
        else:
            assert a.type is kind, (name, a.type)
    need = [x for name in REQUIRED for x in (f"--{name}", "v")]
    args = parser.parse_args(need + ["--fp16", "--max_seq_len", "50", "--log_steps", "10"])
    assert args.fp16 is True and args.max_seq_len == 50 and args.log_steps == 10 and args.max_seq_len_pv is None


def test_without_a_gpu_the_script_says_so(tmp_path):
    """the child sees no GPU whatever the machine has: the refusal comes before any file is read"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    argv = [x for name in REQUIRED for x in (f"--{name}", str(tmp_path / name))]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "coca_pretrain.py")] + argv, capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode != 0
    assert "runs on the MI355X HIP engine only (no CPU path); no GPU is visible" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "output_dir")
