"""What the training scripts share, on the host: the one warm-up/decay schedule and its two forwarding names, the clip-by-norm
arithmetic of the fused optimiser step, dist.Ranks under two gloo CPU processes and in one process, and the rank-0 run set-up of the
BERT scripts (cli_common.rank0_run_logging)."""
import logging
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

SCHEDULES = [(0, 10), (3, 10), (10, 10), (30, 100)]          # (warm-up, total)


@pytest.mark.parametrize("warm,total", SCHEDULES)
def test_schedule_is_transformers_and_the_three_names_agree(warm, total):
    from transformers import get_linear_schedule_with_warmup
    from item_alignment_amd.cli_common import linear_schedule
    from item_alignment_amd.models.kg_pretrain import linear_schedule_lambda
    from item_alignment_amd.train import linear_schedule_with_warmup
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = get_linear_schedule_with_warmup(opt, warm, total)
    lam = linear_schedule_lambda(warm, total)
    for step in range(total + 3):
        ours = linear_schedule_with_warmup(step, warm, total)
        assert ours == sch.get_last_lr()[0], (step, ours, sch.get_last_lr()[0])          # base lr 1.0: the factor itself
        assert type(ours) is float and linear_schedule(step, total, warm) == ours and lam(step) == ours
        opt.step()
        sch.step()


class StubArena:
    def __init__(self, grad):
        self.grad, self.calls = grad, []

    def adamw_step(self, lr, **kw):
        self.calls.append(dict(lr=lr, **kw))


@pytest.mark.parametrize("inv_world", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("grad_value", [0.01, 3.0], ids=["below_max_norm", "above_max_norm"])
def test_clipped_adamw_step_is_the_step_of_bert_pretrain(inv_world, grad_value):
    from item_alignment_amd.cli_common import linear_schedule
    from item_alignment_amd.train import clipped_adamw_step
    args = SimpleNamespace(learning_rate=2e-5, max_grad_norm=1.0, warmup_steps=3, adam_epsilon=1e-8)
    global_steps, total_steps = 2, 10
    # the SUM over 1 / inv_world ranks, as GradBucketReducer.finish() leaves it in the arena
    arena = StubArena(torch.full((64,), grad_value / inv_world))
    assert (arena.grad.norm().item() * inv_world < args.max_grad_norm) == (grad_value == 0.01)
    lr = args.learning_rate * linear_schedule(global_steps - 1, total_steps, args.warmup_steps)
    clipped_adamw_step(arena, lr, args.max_grad_norm, inv_world, betas=(0.9, 0.999), eps=args.adam_epsilon, weight_decay=0.0)
    # bert_pretrain.py's step before it was shared, literally
    norm = arena.grad.norm().item() * inv_world
    scale = min(1.0, args.max_grad_norm / (norm + 1e-6)) * inv_world
    want_lr = args.learning_rate * (1 / max(1, 3))
    assert arena.calls == [dict(lr=want_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=scale)]
    assert (scale == inv_world) == (grad_value == 0.01)          # no clipping below the bound: only the averaging is left
    arena = StubArena(torch.ones(4))
    clipped_adamw_step(arena, 0.5, 2.0, betas=(0.8, 0.7), eps=1e-3, weight_decay=0.25)
    assert arena.calls == [dict(lr=0.5, betas=(0.8, 0.7), eps=1e-3, weight_decay=0.25, grad_scale=min(1.0, 2.0 / (2.0 + 1e-6)))]


def test_arena_adamw_passes_its_betas_and_weight_decay():
    from item_alignment_amd.train import ArenaAdamW
    arena = StubArena(None)
    ArenaAdamW(SimpleNamespace(param_arena=arena), 1e-3, 1e-8, 1e-5).step(0.5, grad_scale=0.25)
    ArenaAdamW(SimpleNamespace(param_arena=arena), 1e-3, 1e-6, 0.0, betas=(0.9, 0.999)).step(1.0)
    assert arena.calls == [dict(lr=5e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-5, grad_scale=0.25),
                           dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, grad_scale=1.0)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_worker(rank, world, port, out, fail):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from item_alignment_amd import dist as iadist
    ranks = iadist.Ranks()
    got = dict(before=(ranks.rank, ranks.world, ranks.dp, dist.is_initialized()))
    try:
        ranks.init("cpu")
        got["device"] = str(ranks.device)
        five = (torch.arange(5), torch.arange(10).reshape(5, 2))
        got["cut5"] = [t.tolist() for t in ranks.cut(five)]
        got["cut1"] = ranks.cut((torch.arange(1),))
        got["seed"] = ranks.seed(12345)
        got["mean"] = ranks.mean(torch.tensor(1.0 if rank == 0 else 3.0))
        got["mean_in_dtype"] = ranks.mean(torch.tensor(1.0 if rank == 0 else 3.0), in_dtype=True)
        ranks.written()
        got["initialized_inside"] = dist.is_initialized()
        if fail:
            raise RuntimeError("inside the run")
    except RuntimeError as e:
        got["raised"] = str(e)
    finally:
        ranks.close()
    got["initialized_after"] = dist.is_initialized()
    out[rank] = got


@pytest.mark.parametrize("fail", [False, True], ids=["clean_exit", "exception_inside_the_run"])
def test_ranks_under_two_gloo_processes(fail):
    from item_alignment_amd import dist as iadist
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, _free_port(), out, fail), nprocs=world, join=True)
    got = dict(out)
    assert sorted(got) == [0, 1]
    rows = torch.arange(5)
    for rank in (0, 1):
        g = got[rank]
        lo, hi = iadist.deal_rows(5, rank, world)
        assert g["before"] == (rank, world, True, False) and g["device"] == "cpu"
        assert g["cut5"] == [rows[lo:hi].tolist(), torch.arange(10).reshape(5, 2)[lo:hi].tolist()]
        assert g["cut1"] is None                                   # fewer rows than ranks: both skip
        assert g["mean"] == 2.0 and g["mean_in_dtype"] == 2.0
        assert g["initialized_inside"] is True and g["initialized_after"] is False
        assert g.get("raised") == ("inside the run" if fail else None)
    assert got[0]["cut5"][0] + got[1]["cut5"][0] == rows.tolist()      # the slices in rank order are the batch
    assert got[0]["seed"] == 12345 and got[1]["seed"] != 12345 and 0 <= got[1]["seed"] < 2 ** 32


def test_ranks_in_one_process_is_the_identity(monkeypatch):
    from item_alignment_amd import dist as iadist
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(iadist, "FORCE", False)
    ranks = iadist.Ranks().init("cpu")
    try:
        assert (ranks.rank, ranks.world, ranks.local, ranks.dp, ranks.created) == (0, 1, 0, False, False)
        assert not dist.is_initialized() and ranks.device == torch.device("cpu")
        batch = [torch.arange(3), torch.arange(0)]
        assert ranks.cut(batch) is batch and ranks.cut((torch.arange(0),)) is not None
        assert ranks.attach(SimpleNamespace()) is None
        assert ranks.seed(12345) == 12345
        value = torch.tensor(1.5)
        assert ranks.mean(value) == 1.5 and ranks.mean(value, in_dtype=True) == 1.5
        ranks.written()
        assert not dist.is_initialized()
    finally:
        ranks.close()
    assert not dist.is_initialized()


def _lines(path):
    with open(path) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("fail", [False, True], ids=["clean_exit", "exception_inside"])
def test_rank0_run_logging_adds_and_removes_its_handlers(tmp_path, capsys, fail):
    from item_alignment_amd.cli_common import rank0_run_logging
    log = logging.getLogger(f"test_train_harness.rank0.{fail}")
    path = tmp_path / "run.log"
    held = []
    for message in ("first", "second"):          # entered twice, as a test that calls main() twice does
        try:
            with rank0_run_logging(log, 0, str(path), str(tmp_path / "tf-logs")) as writer:
                handlers = list(log.handlers)
                held.append(handlers)
                assert [type(h) for h in handlers] == [logging.FileHandler, logging.StreamHandler]
                assert log.level == logging.INFO and log.propagate is False
                assert writer is None or hasattr(writer, "add_scalar")
                log.info(message)
                log.debug("not shown")
                if fail:
                    raise RuntimeError("inside")
        except RuntimeError:
            assert fail
        assert log.handlers == []
        assert handlers[0].stream is None or handlers[0].stream.closed          # FileHandler.close() drops its stream
    text = _lines(path)
    assert len(text) == 2 and text[0].endswith(" - INFO - first") and text[1].endswith(" - INFO - second")          # every line once
    shown = [line for line in capsys.readouterr().out.splitlines() if log.name in line]
    assert len(shown) == 2


def test_rank0_run_logging_on_another_rank(tmp_path, capsys):
    from item_alignment_amd.cli_common import rank0_run_logging
    log = logging.getLogger("test_train_harness.rank1")
    with rank0_run_logging(log, 1, str(tmp_path / "run.log"), str(tmp_path / "tf-logs")) as writer:
        assert writer is None and log.level == logging.WARNING
        assert [type(h) for h in log.handlers] == [logging.StreamHandler]
        log.info("quiet")
        log.warning("loud")
    assert log.handlers == [] and not (tmp_path / "run.log").exists() and not (tmp_path / "tf-logs").exists()
    shown = [line for line in capsys.readouterr().out.splitlines() if log.name in line]
    assert len(shown) == 1 and shown[0].endswith(" - WARNING - loud")
