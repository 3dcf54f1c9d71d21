"""NormFreeNet.embed, the tower's forward-only path (activation epilogues in the direct 3x3 kernels, SiLU + pool in one read, held
standardised weights, per-(batch, size) buffers), and image_embedding.py end to end.

Parity: eca_nfnet_l0 / l1 with seeded weights (oracle/weights.py draws every gain around 1, conv3's included, so the residual branches
carry signal) against the fp32 restatement in oracle/ref_models.py.  The yardstick is the existing forward's own rel-rms error against
the same oracle on the same inputs: embed rounds strictly less often (no bf16 store between a 3x3 convolution and its SiLU, none between
final_act and the pool), so its error may be at most 1.5 x that -- a margin for sample noise at 3 x 2304 outputs, not for a systematic
gap.  Figures seen on one MI355X are in profiles/nfnet_embed_parity.json (IA_WRITE_PROFILES=1 rewrites it; no input to any check).

Images of 64 x 64 (maps 16 / 8 / 4 / 2) and 100 x 100 (25 / 13 / 7 / 4: every ceil-mode size); batches of 3, then 2 (a prefix of the
same plan's buffers), then the first batch again on the reused buffers: bit-identical, so the borders zeroed once are still zero.
The tower retains ONE plan: another image size or a larger batch rebuilds it, and what it holds does not grow with the number of
distinct batch sizes a run meets (test_one_plan_is_retained)."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOWERS = ["eca_nfnet_l0", "eca_nfnet_l1"]
SIZES = (64, 100)
MARGIN = 1.5
PARITY = {}


def rel_rms(got, want):
    got, want = got.double().cpu(), want.double()
    return float((got - want).norm() / want.norm())


def build(name, sd):
    from item_alignment_amd.models.nfnet import create_nfnet
    net = create_nfnet(name)
    missing, unexpected = net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("head.fc") for k in missing), (missing, unexpected)
    return net.cuda().eval()


@pytest.fixture(scope="module", params=TOWERS)
def tower(request, gpu):
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    name = request.param
    ncfg = O.nfnet_cfg(name)
    sd = seeded_state_dict(O.nfnet_state_spec(ncfg, prefix="e"), 31, scale=0.5)
    return name, ncfg, sd, build(name, sd)


def test_embed_against_the_oracle(tower):
    from oracle import ref_models as O
    name, ncfg, sd, net = tower
    g = torch.Generator().manual_seed(17)
    plan = None
    for size in SIZES:
        first = None
        for B in (3, 2):
            images = torch.randn((B, 3, size, size), generator=g)
            with torch.no_grad():
                ref = O.nfnet_global_pool(O.nfnet_forward_features(sd, "e", ncfg, images))
                fwd = net(images.cuda())
            emb = net.embed(images.cuda())
            assert tuple(emb.shape) == (B, net.num_features) and emb.dtype == torch.float32
            if B == 3:                                                  # another image size: the plan was rebuilt
                assert net.__dict__["_embed_plan_held"] is not plan
                plan = net.__dict__["_embed_plan_held"]
            assert net.__dict__["_embed_plan_held"] is plan and plan.capacity == 3 and plan.key[:2] == (size, size)
            e_fwd, e_emb = rel_rms(fwd, ref), rel_rms(emb, ref)
            PARITY["%s %dx%d B=%d" % (name, size, size, B)] = {"forward_rel_rms": e_fwd, "embed_rel_rms": e_emb}
            print("%s %3d x %3d B = %d: rel-rms error against fp32  forward %.3e  embed %.3e  (ratio %.2f)" % (name, size, size, B, e_fwd, e_emb, e_emb / e_fwd))
            assert e_fwd < 5e-2, e_fwd                                  # the yardstick itself is sound
            assert e_emb <= MARGIN * e_fwd, (name, size, B, e_emb, e_fwd)
            if first is None:
                first = (images, emb.clone())
        again = net.embed(first[0].cuda())                             # the plan's buffers, used again after a smaller batch
        assert net.__dict__["_embed_plan_held"] is plan
        assert torch.equal(again, first[1])
    if os.environ.get("IA_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "nfnet_embed_parity.json")
        old = json.load(open(path)) if os.path.isfile(path) else {}
        old.update(PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")


def test_one_plan_is_retained(tower):
    """what embed keeps is bounded by the largest batch at the current size: smaller batches (a batch with unreadable images left out,
    the last partial one) run in a prefix of the same buffers and give what a plan of their own size gives, a larger batch or another
    size replaces the plan -- and returns the old one's memory.  (Every comparison is between runs of ONE batch size.  The tower's existing
    kernels do not give an image the same bits in batches of every size: measured on eca_nfnet_l0 at 64 x 64, images 0 and 1 are
    bit-identical in batches of 2, 3 and 4, image 2 differs between a batch of 3 and one of 4 by up to 1.2e-2 -- through forward
    exactly as through embed, so it is not the plan's doing; tests/test_models_gpu.py test_nfnet_two_tower_chunked_batch_equals_whole
    compares chunked and whole batches with tolerances for the same reason.)"""
    name, ncfg, sd, _ = tower
    net = build(name, sd)
    x = torch.randn((4, 3, 64, 64), generator=torch.Generator().manual_seed(9)).cuda()
    alone = {B: build(name, sd).embed(x[:B]).clone() for B in (1, 2, 4)}         # plans of exactly that size
    e3 = net.embed(x[:3]).clone()
    plan = net.__dict__["_embed_plan_held"]
    held = plan.nbytes()
    for B in (2, 1, 3, 2):
        out = net.embed(x[:B])
        assert net.__dict__["_embed_plan_held"] is plan and plan.nbytes() == held, B
        assert torch.equal(out, alone[B] if B in alone else e3), B
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    e4 = net.embed(x)                                                            # a larger batch: rebuilt, the old plan gone
    plan4 = net.__dict__["_embed_plan_held"]
    assert plan4 is not plan and plan4.capacity == 4 and "_embed_plans" not in net.__dict__
    assert torch.equal(e4, alone[4])
    assert held < plan4.nbytes() <= 2 * held                                     # per-image buffers: about 4 / 3 of the old plan
    del plan
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert grown <= plan4.nbytes() - held + (8 << 20), (grown, plan4.nbytes(), held)   # the old plan was not kept beside the new one
    net.embed(torch.randn((2, 3, 100, 100), generator=torch.Generator().manual_seed(4)).cuda())
    assert net.__dict__["_embed_plan_held"].key[:2] == (100, 100) and net.__dict__["_embed_plan_held"].capacity == 2


def test_fallbacks_are_logged_and_right(gpu, monkeypatch, caplog):
    """no shipped configuration lacks an activation-epilogue kernel; forced here.  Two blocks declared not direct run through their
    existing forward in the middle of the chain (fresh tensors between plan-owned ones); the first block declared not direct sends the
    whole call through forward.  Held to the same yardstick as embed, and logged once per tower."""
    import logging
    from types import SimpleNamespace
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    from item_alignment_amd.models.nfnet import NormFreeBlock, NormFreeNet
    ncfg = SimpleNamespace(depths=(1, 2, 1, 1), channels=(256, 512, 512, 512), stem_chs=128, group_size=64, bottle_ratio=0.25, num_features=512, alpha=0.2,
                           attn_gain=2.0, eps=1e-5, ch_div=8)
    sd = seeded_state_dict(O.nfnet_state_spec(ncfg, prefix="e"), 21, scale=0.5)
    net = NormFreeNet(ncfg.depths, ncfg.channels, 1.0)
    net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    net = net.cuda().eval()
    images = torch.randn((3, 3, 100, 100), generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        ref = O.nfnet_global_pool(O.nfnet_forward_features(sd, "e", ncfg, images))
        fwd = net(images.cuda()).clone()
    direct = net.embed(images.cuda()).clone()
    blocks = [b for st in net.stages for b in st]
    real = NormFreeBlock.embed_direct
    for off in ({1, 3}, {0}):
        net._drop_embed_state()
        net.__dict__.pop("_embed_fallback_logged", None)
        monkeypatch.setattr(NormFreeBlock, "embed_direct", lambda self, B, H, W: blocks.index(self) not in off and real(self, B, H, W))
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            got = net.embed(images.cuda()).clone()
            assert torch.equal(net.embed(images.cuda()), got)
        assert caplog.text.count("no activation-epilogue kernel") == 1, caplog.text
        if off == {0}:
            assert torch.equal(got, fwd)                                # the existing launches, all of them
        else:
            assert not torch.equal(got, direct) and not torch.equal(got, fwd)
            assert rel_rms(got, ref) <= MARGIN * rel_rms(fwd, ref), (rel_rms(got, ref), rel_rms(fwd, ref))
    monkeypatch.setattr(NormFreeBlock, "embed_direct", real)
    assert rel_rms(direct, ref) <= MARGIN * rel_rms(fwd, ref)


def test_a_changed_weight_is_never_served_stale(tower):
    name, ncfg, sd, _ = tower
    net = build(name, sd)
    x = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(3)).cuda()
    e1 = net.embed(x).clone()
    assert torch.equal(net.embed(x), e1)
    # (a) an in-place write torch sees: the arena's staleness guard refreshes, the held weights go
    with torch.no_grad():
        net.stem.conv2.weight[1, 2, 0, 1] += 0.75
    e2 = net.embed(x).clone()
    assert not torch.equal(e2, e1)
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["e.stem.conv2.weight"][1, 2, 0, 1] += 0.75
    assert torch.equal(build(name, sd2).embed(x), e2)
    # (b) a write into the arena's master behind torch's back, announced by refresh_shadow() as arena.py asks
    w = net.stages[0][0].conv2b.weight
    w.data[5, 7, 1, 1] -= 0.5
    net.param_arena.refresh_shadow()
    e3 = net.embed(x).clone()
    assert not torch.equal(e3, e2)
    sd2["e.stages.0.0.conv2b.weight"][5, 7, 1, 1] -= 0.5
    assert torch.equal(build(name, sd2).embed(x), e3)
    # (c) load_state_dict brings the first weights back
    net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    assert "_embed_held" not in net.__dict__
    assert torch.equal(net.embed(x), e1)


def test_training_after_embed_is_bit_identical(gpu):
    """train() then forward / backward on a tower that served embed calls = on one that never did"""
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    ncfg = O.nfnet_cfg("eca_nfnet_l0")
    sd = seeded_state_dict(O.nfnet_state_spec(ncfg, prefix="e"), 31, scale=0.5)
    g = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 64, 64), generator=g).cuda()
    wts = torch.randn((2, 2304), generator=g).cuda()
    outs = []
    for use_embed in (True, False):
        net = build("eca_nfnet_l0", sd)
        if use_embed:
            net.embed(x)
            net.embed(x[:1])
        net.train()
        assert "_embed_held" not in net.__dict__ and "_embed_plans" not in net.__dict__
        net.param_arena.zero_grad()
        out = net(x)
        (out * wts).sum().backward()
        torch.cuda.synchronize()
        outs.append((out.detach().clone(), net.param_arena.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert float(outs[0][1].abs().max()) > 0


def test_image_embedding_script_end_to_end(gpu, tmp_path):
    """eight generated JPEGs of 96 x 96 through image_embedding.py with eca_nfnet_l0 at --image_size 64 --batch_size 3, decoded by Pillow and
    by the GPU (--gpu_jpeg): the same keys, the same values wherever the GPU decode is byte-exact (checked per image), features and not
    zeros, and the last partial batch gets features like the others"""
    import numpy as np
    from PIL import Image
    import image_embedding as IE
    from item_alignment_amd.data.datasets import load_image
    from item_alignment_amd.data.gpu_preproc import GpuImagePipeline
    from item_alignment_amd.data.transforms import ImageTransform
    from item_alignment_amd.models.nfnet import create_nfnet
    data = tmp_path / "data"
    (data / "item_images_cropped").mkdir(parents=True)
    rs = np.random.RandomState(11)
    ids = ["it%02d" % i for i in range(8)]
    yy, xx = np.mgrid[0:96, 0:96]
    with open(data / "item_info.jsonl", "w", encoding="utf-8") as w:
        for n, i in enumerate(ids):
            w.write(json.dumps({"item_id": i}) + "\n")
            img = np.stack([(yy * (n + 1) + xx) % 256, (xx * 2 + 30 * n) % 256, (yy + xx * n) % 256], -1) + rs.randint(-20, 20, (96, 96, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(data / "item_images_cropped" / f"{i}.jpg", quality=92)
    torch.manual_seed(5)
    net = create_nfnet("eca_nfnet_l0")
    with torch.no_grad():
        for blk in (b for st in net.stages for b in st):
            blk.conv3.gain.fill_(1.0)
    ckpt = tmp_path / "tower.bin"
    torch.save({"img_encoder." + k: v for k, v in net.state_dict().items()} | {"classifier.dense.weight": torch.zeros(4, 4)}, ckpt)
    common = ["--data_dir", str(data), "--cv_model_name", "eca_nfnet_l0", "--pretrained_model_path", str(ckpt), "--image_size", "64", "--batch_size", "3"]
    IE.main(common + ["--output_dir", str(tmp_path / "host")])
    IE.main(common + ["--output_dir", str(tmp_path / "gpu"), "--gpu_jpeg"])
    host = json.load(open(tmp_path / "host" / "image_embedding.json"))
    dev = json.load(open(tmp_path / "gpu" / "image_embedding.json"))
    assert list(host) == ids and list(dev) == ids
    pipe, tf = GpuImagePipeline(64, "cuda"), ImageTransform(64, False)
    exact = 0
    for i in ids:
        path = str(data / "item_images_cropped" / f"{i}.jpg")
        assert len(host[i]) == 2304 and any(v != 0.0 for v in host[i]) and all(np.isfinite(host[i]))
        frame = pipe.decode([load_image(path, tf, jpeg=True)])[0].u8.cpu().numpy()
        if np.array_equal(frame, np.array(Image.open(path).convert("RGB"))):
            exact += 1
            assert dev[i] == host[i], i
        else:
            assert np.allclose(dev[i], host[i], rtol=0.1, atol=0.05), i
    assert exact >= 1, "no image was decoded byte-exactly: the comparison above checked nothing"
    assert host[ids[0]] != host[ids[7]]
