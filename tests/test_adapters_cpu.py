"""CPU tests of the device-resident adapter path: lora.read_adapter on adapter directories written here, and the model-level
switching logic (load_adapter / set_adapter / unload_adapter / active_adapter) over tests/fake_engine, whose three new engine
methods are attached here as recorders."""
import json
import os

import numpy as np
import pytest
import torch

import fake_engine
from test_dropin_cpu import TOK, checkpoint_dir  # noqa: F401  (checkpoint_dir: fixture)
from test_oracle_golden import G as GOLD
from test_prompt_prefix_cpu import PrefixFakeEngine, _inputs
from vibevoice_amd import lora

Q0 = "layers.0.self_attn.q_proj"            # [128, 128] in the tiny model
D1 = "layers.1.mlp.down_proj"               # [128, 256]
HG = "layers.0.ffn.gate_proj"               # head: [384, 128]
SHAPES = {Q0: (128, 128), D1: (128, 256), HG: (384, 128)}


def _pair(mod, r, seed):
    g = torch.Generator().manual_seed(seed)
    n, k = SHAPES[mod]
    return torch.randn(r, k, generator=g), torch.randn(n, r, generator=g)


def _write(root, lm=None, head=None, lm_cfg=None, head_cfg=None, head_prefix="base."):
    """<root>/lora/adapter_* and <root>/lora/diffusion_head/adapter_*, as the reference's trainer writes them (torch.save)"""
    d = root / "lora"
    (d / "diffusion_head").mkdir(parents=True, exist_ok=True)
    if lm is not None:
        sd = {}
        for mod, (a, b) in lm.items():
            sd[f"base_model.model.{mod}.lora_A.weight"] = a
            sd[f"base_model.model.{mod}.lora_B.weight"] = b
        torch.save(sd, str(d / "adapter_model.bin"))
        (d / "adapter_config.json").write_text(json.dumps(lm_cfg or {"r": 8, "lora_alpha": 32}))
    if head is not None:
        sd = {}
        for mod, (a, b) in head.items():
            sd[f"base_model.model.{head_prefix}{mod}.lora_A.default.weight"] = a
            sd[f"base_model.model.{head_prefix}{mod}.lora_B.default.weight"] = b
        torch.save(sd, str(d / "diffusion_head" / "adapter_model.bin"))
        (d / "diffusion_head" / "adapter_config.json").write_text(json.dumps(head_cfg or {"r": 4, "lora_alpha": 4}))
    return str(root)


EXPECTED = {"lm." + Q0 + ".weight": 128 * 128, "lm." + D1 + ".weight": 128 * 256, "head." + HG + ".weight": 384 * 128}


# ---------------------------------------------------------------- read_adapter
def test_read_adapter_language_model_alone(tmp_path):
    lm = {Q0: _pair(Q0, 8, 1), D1: _pair(D1, 8, 2)}
    got = lora.read_adapter(_write(tmp_path / "a", lm=lm), EXPECTED)
    assert sorted(got) == ["lm." + Q0 + ".weight", "lm." + D1 + ".weight"]
    for mod, (a, b) in lm.items():
        ga, gb, scale = got["lm." + mod + ".weight"]
        assert ga.dtype == gb.dtype == torch.float32 and torch.equal(ga, a) and torch.equal(gb, b) and scale == 32 / 8
    assert sorted(lora.read_adapter(_write(tmp_path / "a", lm=lm))) == sorted(got)          # the shape check is optional


def test_read_adapter_language_model_and_head_with_the_base_prefix_and_rslora(tmp_path):
    lm = {Q0: _pair(Q0, 8, 3)}
    head = {HG: _pair(HG, 4, 4)}
    p = _write(tmp_path / "b", lm=lm, head=head, head_cfg={"r": 4, "lora_alpha": 6, "use_rslora": True})
    got = lora.read_adapter(p, EXPECTED)
    assert sorted(got) == ["head." + HG + ".weight", "lm." + Q0 + ".weight"]
    ga, gb, scale = got["head." + HG + ".weight"]                      # peft saw the head through the shim's `base` attribute
    assert torch.equal(ga, head[HG][0]) and torch.equal(gb, head[HG][1]) and scale == 6 / 4 ** 0.5
    assert got["lm." + Q0 + ".weight"][2] == 4.0
    # bf16 factors on disk are upcast (peft's autocast_adapter_dtype)
    half = {HG: tuple(t.to(torch.bfloat16) for t in head[HG])}
    got = lora.read_adapter(_write(tmp_path / "c", head=half), EXPECTED)
    assert got["head." + HG + ".weight"][0].dtype == torch.float32
    assert torch.equal(got["head." + HG + ".weight"][0], half[HG][0].float())


def test_read_adapter_refusals(tmp_path):
    lm = {Q0: _pair(Q0, 8, 5)}
    # full-tensor assets
    for i, rel in enumerate(("diffusion_head/diffusion_head_full.bin", "diffusion_head_full.bin", "acoustic_connector/pytorch_model.bin",
                             "semantic_connector/pytorch_model.bin")):
        p = _write(tmp_path / f"full{i}", lm=lm)
        f = os.path.join(p, "lora", rel)
        os.makedirs(os.path.dirname(f), exist_ok=True)
        torch.save({"fc1.weight": torch.ones(2, 2)}, f)
        with pytest.raises(ValueError, match=os.path.basename(rel)) as ei:
            lora.read_adapter(p, EXPECTED)
        assert "load_lora_assets" in str(ei.value)
    # fan_in_fan_out
    p = _write(tmp_path / "fifo", lm=lm, lm_cfg={"r": 8, "lora_alpha": 32, "fan_in_fan_out": True})
    with pytest.raises(ValueError, match="adapter_config.json.*fan_in_fan_out.*load_lora_assets"):
        lora.read_adapter(p, EXPECTED)
    # a pair that does not fit its parameter; ranks that do not match; a module the engine does not have
    a, b = _pair(Q0, 8, 6)
    with pytest.raises(ValueError, match="q_proj.*load_lora_assets"):
        lora.read_adapter(_write(tmp_path / "shape", lm={Q0: (a[:, :64].contiguous(), b)}), EXPECTED)
    with pytest.raises(ValueError, match="q_proj.*rank.*load_lora_assets"):
        lora.read_adapter(_write(tmp_path / "rank", lm={Q0: (a[:4].contiguous(), b)}), EXPECTED)
    with pytest.raises(ValueError, match="layers.7.*load_lora_assets"):
        lora.read_adapter(_write(tmp_path / "nomod", lm={"layers.7.self_attn.q_proj": (a, b)}), EXPECTED)
    # non-finite factors
    bad = a.clone()
    bad[3, 5] = float("nan")
    with pytest.raises(ValueError, match="q_proj.*non-finite.*load_lora_assets"):
        lora.read_adapter(_write(tmp_path / "nan", lm={Q0: (bad, b)}), EXPECTED)
    bad = b.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        lora.read_adapter(_write(tmp_path / "inf", lm={Q0: (a, bad)}), EXPECTED)
    with pytest.raises(FileNotFoundError):
        lora.read_adapter(str(tmp_path / "missing"))


# ---------------------------------------------------------------- the switching logic
@pytest.fixture()
def model(monkeypatch, checkpoint_dir):  # noqa: F811
    from vibevoice_amd import modeling
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(modeling, "Engine", PrefixFakeEngine)
        m = modeling.VibeVoiceForConditionalGenerationInference.from_pretrained(checkpoint_dir, torch_dtype=torch.float32, device_map="cuda")
        m.eval()
        m.set_ddpm_inference_steps(num_steps=5)
        yield m


def _record(model):
    """the three new engine methods as recorders: (op, parameter, ...) in call order; closing the lanes is logged too"""
    log = []
    eng = model.engine
    eng.lora_merge = lambda name, a, b, scale, merge_dtype="float32": log.append(("merge", name, a, b, scale, merge_dtype))
    eng.lora_reset = lambda name=None: log.append(("reset", name))
    eng.weight_read = lambda name, shape: log.append(("read", name))
    close = model.close_lanes

    def close_lanes():
        log.append(("close_lanes",))
        close()
    model.close_lanes = close_lanes
    sync = eng.sync

    def synced():
        log.append(("sync",))
        sync()
    eng.sync = synced
    return log


def test_set_adapter_switching_logic(model, tmp_path):
    x_lm = {Q0: _pair(Q0, 8, 11), D1: _pair(D1, 8, 12)}
    x_hd = {HG: _pair(HG, 4, 13)}
    y_lm = {Q0: _pair(Q0, 8, 14)}
    assert model.load_adapter("x", _write(tmp_path / "x", lm=x_lm, head=x_hd)) == ["head." + HG + ".weight", "lm." + Q0 + ".weight", "lm." + D1 + ".weight"]
    model.load_adapter("y", _write(tmp_path / "y", lm=y_lm), merge_dtype="bfloat16")
    assert model.active_adapter is None
    log = _record(model)
    z = np.load(os.path.join(GOLD, "generate_norefresh_b1.npz"))
    inputs = _inputs(z)
    torch.manual_seed(int(z["seed"]))
    prefix = model.build_prompt_prefix(**inputs)
    e0 = model.weights_epoch
    log.clear()
    model._lanes = [model.fork()]
    lane_engine = model._lanes[0].engine

    # X: its pairs are merged, after the lanes were closed, with one sync at the end
    model.set_adapter("x")
    assert model.active_adapter == "x" and model._lanes == [] and getattr(lane_engine, "closed", False)
    assert log[0] == ("close_lanes",) and log[-1] == ("sync",) and [e[0] for e in log].count("sync") == 1
    merges = {e[1]: e for e in log if e[0] == "merge"}
    assert sorted(merges) == ["head." + HG + ".weight", "lm." + Q0 + ".weight", "lm." + D1 + ".weight"] and len(log) == 5
    _, _, a, b, scale, md = merges["lm." + Q0 + ".weight"]
    assert torch.equal(a, x_lm[Q0][0]) and torch.equal(b, x_lm[Q0][1]) and scale == 4.0 and md == "float32"
    assert merges["head." + HG + ".weight"][4] == 1.0
    assert model.weights_epoch == e0 + 1
    with pytest.raises(RuntimeError, match="stale"):                 # a prefix built under the base weights is refused
        model.generate(**inputs, prompt_prefix=prefix, cfg_scale=1.3, tokenizer=TOK, max_new_tokens=2, show_progress_bar=False)

    # the active adapter again: nothing happens
    log.clear()
    model.set_adapter("x")
    assert log == [] and model.weights_epoch == e0 + 1

    # Y: what X touched and Y does not is reset, then Y's pairs are merged
    model.set_adapter("y")
    ops = [e[:2] for e in log]
    assert ops[0] == ("close_lanes",) and ops[-1] == ("sync",)
    assert sorted(ops[1:3]) == [("reset", "head." + HG + ".weight"), ("reset", "lm." + D1 + ".weight")]
    assert ops[3] == ("merge", "lm." + Q0 + ".weight") and len(ops) == 5
    assert torch.equal(log[3][2], y_lm[Q0][0]) and log[3][5] == "bfloat16"
    assert model.active_adapter == "y" and model.weights_epoch == e0 + 2

    # None: everything the active adapter touched is reset
    log.clear()
    model.set_adapter(None)
    assert [e[:2] for e in log] == [("close_lanes",), ("reset", "lm." + Q0 + ".weight"), ("sync",)]
    assert model.active_adapter is None and model.weights_epoch == e0 + 3
    log.clear()
    model.set_adapter(None)
    assert log == []

    # names
    with pytest.raises(KeyError):
        model.set_adapter("nobody")
    with pytest.raises(KeyError):
        model.unload_adapter("nobody")
    model.set_adapter("y")
    with pytest.raises(ValueError, match="active"):
        model.unload_adapter("y")
    model.unload_adapter("x")
    with pytest.raises(KeyError):
        model.set_adapter("x")
    assert model.active_adapter == "y"
    with pytest.raises(ValueError, match="merge_dtype"):
        model.load_adapter("z", str(tmp_path / "x"), merge_dtype="float16")


def test_load_adapter_checks_the_pairs_against_the_engine(model, tmp_path):
    a, b = _pair(Q0, 8, 21)
    with pytest.raises(ValueError, match="q_proj.*load_lora_assets"):
        model.load_adapter("bad", _write(tmp_path / "bad", lm={Q0: (a[:, :32].contiguous(), b)}))
    assert model.active_adapter is None
    with pytest.raises(KeyError):
        model.set_adapter("bad")
