"""`item_alignment_amd.optim.LAMB` and `ParamArena.lamb_step` on the small two-tower golden model of tests/test_optim_gpu.py.  The
optimiser is isolated from the model's own run-to-run noise (the embedding gradients are fp32 atomic adds in arrival order): every
step is compared with the fp64 reference FED THE GPU'S OWN GRADIENTS AND STATE of that step, and where two runs must agree bit for
bit the second run is handed the first run's gradient arenas."""
import numpy as np
import pytest
import torch

import lamb_reference as R
from golden_util import load_case
from test_optim_gpu import fresh, grouped, linear_schedule_with_warmup, two_tower_args

pytestmark = pytest.mark.gpu

LR, WD, BETAS, EPS = 2e-3, 0.01, (0.9, 0.999), 1e-6


def lamb_groups(model):
    """the BERT recipe: biases and LayerNorm weights are neither decayed nor adapted"""
    groups = grouped(model, WD)
    groups[1]["adapt"] = False
    return groups


def snapshot(arena):
    torch.cuda.synchronize()
    return {k: getattr(arena, k).detach().cpu().numpy().copy() for k in ("master", "grad", "exp_avg", "exp_avg_sq")}


def group_tensors(arena, group):
    name_of = {id(p): n for n, p in zip(arena.names, arena.params)}
    offset_of = {id(p): o for p, o in zip(arena.params, arena.offsets)}
    out = []
    for p in group["params"]:
        x = R.Tensor(name_of[id(p)], p.numel(), bool(group["adapt"]))
        x.decay, x.off = True, offset_of[id(p)]                 # the group's weight_decay applies to every tensor of the group
        out.append(x)
    return out


def named_ratios(arena, optimizer):
    name_of = {id(p): n for n, p in zip(arena.names, arena.params)}
    return {name_of[id(p)]: r for p, r in optimizer.trust_ratios().items()}


def backward(model, args, step):
    from item_alignment_amd.models import functional as Fn
    Fn.set_step_seed(step)
    loss = model(**args).loss
    loss.backward()
    return loss


@pytest.mark.parametrize("build_before_cuda", [True, False])
def test_three_scheduled_steps_follow_the_reference_group_by_group(gpu, build_before_cuda):
    from item_alignment_amd.optim import LAMB
    case = load_case("roberta_two_tower_ce")
    args = two_tower_args(case)
    model = fresh(case)
    if not build_before_cuda:
        model.cuda()
        model.ensure_arena()
    optimizer = LAMB(lamb_groups(model), lr=LR, betas=BETAS, eps=EPS)
    scheduler = linear_schedule_with_warmup(optimizer, 2, 8)
    if build_before_cuda:
        model.cuda()
    model.eval()                                            # dropout off: not needed for the comparison, keeps the losses comparable
    arena = model.param_arena
    for step in range(3):
        optimizer.zero_grad()
        backward(model, args, step)
        before = snapshot(arena)
        lrs = [g["lr"] for g in optimizer.param_groups]
        assert lrs[0] == pytest.approx(LR * min(1.0, step / 2))
        optimizer.step()
        scheduler.step()
        after = snapshot(arena)
        ratios = named_ratios(arena, optimizer)
        assert len(ratios) == len(arena.params)
        for group, lr in zip(optimizer.param_groups, lrs):
            tensors = group_tensors(arena, group)
            hp = R.Hyper(lr=lr, b1=BETAS[0], b2=BETAS[1], eps=EPS, wd=group["weight_decay"])
            _, exp = R.reference_step(tensors, before["master"], before["grad"], before["exp_avg"], before["exp_avg_sq"], hp, step + 1)
            R.check_step(f"optim.LAMB step {step + 1} wd {group['weight_decay']} adapt {group['adapt']}", tensors, exp, after["master"],
                         after["exp_avg"], after["exp_avg_sq"], ratios)
            if not group["adapt"]:
                assert all(ratios[x.name] == 1.0 for x in tensors)
            else:
                assert sum(ratios[x.name] != 1.0 for x in tensors) > len(tensors) // 2
        assert np.array_equal(after["grad"], before["grad"])
        assert torch.equal(arena.shadow.float(), arena.master.to(torch.bfloat16).float())
    assert arena.stale_refreshes == 0 and arena.step_count == 3
    sd = optimizer.state_dict()
    assert set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3
    assert [g["adapt"] for g in sd["param_groups"]] == [True, False]


def test_state_dict_round_trip_and_lamb_step_are_bit_equal_on_equal_gradients(gpu):
    """Run A: four optim.LAMB steps, keeping every step's gradient arena and the state after step 2.  Run B: a new model and optimiser
    loaded from that state, steps 3 and 4 on A's gradients.  Run C: arena.lamb_step, four steps on A's gradients.  Same masters,
    moments and shadow, bit for bit."""
    from item_alignment_amd.optim import LAMB
    case = load_case("roberta_two_tower_ce")
    args = two_tower_args(case)

    a = fresh(case).cuda().eval()
    oa = LAMB(lamb_groups(a), lr=LR, betas=BETAS, eps=EPS)
    grads, mid = [], None
    for step in range(4):
        oa.zero_grad()
        backward(a, args, step)
        grads.append(a.param_arena.grad.clone())
        oa.step()
        if step == 1:
            mid_opt = {k: (v if k != "state" else {i: {kk: vv.clone() if torch.is_tensor(vv) else vv for kk, vv in st.items()}
                                                   for i, st in v.items()}) for k, v in oa.state_dict().items()}
            mid = ({k: v.detach().clone() for k, v in a.state_dict().items()}, mid_opt)
    torch.cuda.synchronize()

    b = fresh(case).cuda().eval()
    b.ensure_arena()
    b.load_state_dict(mid[0])
    b.param_arena.refresh_shadow()
    ob = LAMB(lamb_groups(b), lr=LR * 7, betas=(0.5, 0.5), eps=1.0)          # every hyper-parameter comes back from the state dict
    ob.load_state_dict(mid[1])
    assert all(g["step_count"] == 2 and g["lr"] == LR and tuple(g["betas"]) == BETAS for g in ob.param_groups)
    for step in (2, 3):
        b.param_arena.grad.copy_(grads[step])
        ob.step()

    c = fresh(case).cuda().eval()
    for step in range(4):
        c.param_arena.grad.copy_(grads[step])
        c.param_arena.lamb_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)
    torch.cuda.synchronize()
    names = c.param_arena.last_trust_ratios()
    assert set(names) == set(c.param_arena.names)
    assert all(r == 1.0 for n, r in names.items() if "bias" in n or "LayerNorm.weight" in n)
    assert named_ratios(a.param_arena, oa) == names

    for other, what in ((b, "resumed"), (c, "arena.lamb_step")):
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a.param_arena, k), getattr(other.param_arena, k)), (what, k)
        assert torch.equal(a.param_arena.shadow.view(torch.int16), other.param_arena.shadow.view(torch.int16)), what
