"""The host side of the CLIP text encoder (SD/clip_text.py) against the recorded fixture tests/golden/clip_text.npz and
the float64 model of clip_text_ref_cpu.py: the tokenizer, the module tree and its loader, the errors, the command lines.
No GPU."""
import importlib.util
import json
import os
import random
import sys

import pytest
import torch

import clip_text_ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "train-scripts")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def vocab_dir(golden, tmp_path_factory):
    return R.write_vocab(golden, str(tmp_path_factory.mktemp("clip_vocab")))


@pytest.fixture(scope="module")
def tokenizer(vocab_dir):
    from unlearn_saliency_amd.SD.clip_text import ClipTokenizerLite
    return ClipTokenizerLite(vocab_dir)


def lite(golden, dtype=torch.float64):
    from unlearn_saliency_amd.SD.clip_text import ClipTextLite
    m = ClipTextLite(golden["config"])
    m.load_state_dict(golden["weights"])
    return m.to(dtype).eval()


# ------------------------------------------------------------------------------------------------------ tokenizer
def test_fixture_covers_the_cases(golden):
    ids, prompts, eos = golden["ids"], golden["prompts"], golden["vocab"]["<|endoftext|>"]
    assert ids.shape == (len(prompts), 77) and len(prompts) >= 20
    assert "" in prompts and "a" in prompts and any("\t" in p for p in prompts) and any("é" in p for p in prompts)
    assert any("#" in p for p in prompts) and any(p.startswith("Image of") for p in prompts)
    assert bool((ids[:, 0] == golden["vocab"]["<|startoftext|>"]).all()) and bool((ids[:, -1] == eos).all())
    assert ids[prompts.index("")].tolist() == [golden["vocab"]["<|startoftext|>"]] + [eos] * 76
    full = [i for i, p in enumerate(prompts) if int(ids[i, 75]) != eos or len(p) >= 100]
    assert len(full) >= 3                                        # 75 tokens, 76 tokens, the truncated one


def test_ids_equal_the_fixtures_on_every_prompt(golden, tokenizer):
    got = tokenizer.encode(golden["prompts"])
    assert got.dtype == torch.int64 and got.shape == golden["ids"].shape
    for i, p in enumerate(golden["prompts"]):
        assert got[i].tolist() == golden["ids"][i].tolist(), repr(p)
    assert tokenizer.encode("it's").tolist() == got[golden["prompts"].index("it's")][None].tolist()


def test_ids_equal_transformers_on_random_strings(golden, vocab_dir, tokenizer):
    transformers = pytest.importorskip("transformers")
    hf = transformers.CLIPTokenizer(os.path.join(vocab_dir, "vocab.json"), os.path.join(vocab_dir, "merges.txt"))
    alphabet = "abcdefghijklmnopqrstuvwxyzTHEING0123456789" + "!\"$%&'()*+,-./:;?" + "é#@ü" + "    \t\n"
    rng = random.Random(7)
    texts = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 60))) for _ in range(300)]
    texts += [" ".join(rng.choice(["the", "thing", "image", "of", "chain", "and", "they'll", "it's", "café", "!!!", "10"])
                       for _ in range(rng.randint(1, 90))) for _ in range(100)]
    want = hf(texts, truncation=True, max_length=77, padding="max_length")["input_ids"]
    got = tokenizer.encode(texts)
    for t, a, b in zip(texts, got.tolist(), want):
        assert a == list(b), repr(t)


def test_split_words_follows_the_pattern():
    from unlearn_saliency_amd.SD.clip_text import split_words
    assert split_words("it's they'll x1y22 a--b 'd") == ["it", "'s", "they", "'ll", "x", "1", "y", "2", "2", "a", "--", "b", "'d"]
    assert split_words("  ") == [] and split_words("é!") == ["é", "!"]


def test_missing_file_names_the_path_and_both_files(tmp_path, golden):
    from unlearn_saliency_amd.SD.clip_text import ClipTokenizerLite
    with pytest.raises(FileNotFoundError, match="vocab.json") as e:
        ClipTokenizerLite(str(tmp_path))
    assert str(tmp_path) in str(e.value) and "merges.txt" in str(e.value)
    with open(tmp_path / "vocab.json", "w") as f:
        json.dump(golden["vocab"], f)
    with pytest.raises(FileNotFoundError, match="merges.txt") as e:
        ClipTokenizerLite(str(tmp_path))
    assert "vocab.json and merges.txt" in str(e.value)


# ------------------------------------------------------------------------------------------------------ the model
def test_float64_model_equals_the_fixture(golden):
    ids = golden["ids"][golden["model_prompts"]]
    got = R.forward(golden["weights"], golden["config"], ids)
    scale = float(golden["hidden"].abs().max())
    assert float((got - golden["hidden"]).abs().max()) <= 1e-12 * scale


def test_library_forward_in_float64_equals_the_float64_model(golden):
    ids = golden["ids"][golden["model_prompts"]]
    with torch.no_grad():
        got = lite(golden)(ids)
    want = R.forward(golden["weights"], golden["config"], ids)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_fp32_library_forward_is_at_the_recorded_yardstick(golden):
    ids = golden["ids"][golden["model_prompts"]]
    with torch.no_grad():
        got = lite(golden, torch.float32)(ids).double()
    assert float((got - golden["hidden"]).abs().max()) <= 8 * golden["yardstick"]


def test_load_compvis_strips_the_prefix_and_tolerates_position_ids(golden):
    from unlearn_saliency_amd.SD.clip_text import ClipTextLite
    sd = {"cond_stage_model.transformer." + k: v.clone() for k, v in golden["weights"].items()}
    sd["cond_stage_model.transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    sd["model.diffusion_model.out.2.bias"] = torch.zeros(4)
    sd["first_stage_model.quant_conv.bias"] = torch.zeros(8)
    m = ClipTextLite(golden["config"]).load_compvis({"state_dict": sd})
    for k, v in m.state_dict().items():
        assert torch.equal(v, golden["weights"][k]), k
    assert set(m.state_dict()) == set(golden["weights"])
    bad = dict(sd)
    del bad["cond_stage_model.transformer.text_model.final_layer_norm.bias"]
    with pytest.raises(KeyError, match="final_layer_norm.bias"):
        ClipTextLite(golden["config"]).load_compvis(bad)
    bad = dict(sd)
    bad["cond_stage_model.transformer.text_model.final_layer_norm.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match="final_layer_norm.bias"):
        ClipTextLite(golden["config"]).load_compvis(bad)


def test_v1_parameter_count():
    from unlearn_saliency_amd.SD import ldm_lite
    from unlearn_saliency_amd.SD.clip_text import ClipTextLite
    with torch.device("meta"):
        m = ClipTextLite.v1()
    n = sum(p.numel() for p in m.parameters())
    assert n == 123_060_480
    assert ldm_lite.SD_V1_FROZEN_PARAMS == 83_653_863 + n
    assert "text_model.embeddings.token_embedding.weight" in m.state_dict()
    assert "text_model.encoder.layers.11.mlp.fc2.bias" in m.state_dict()


def test_bad_id_is_a_value_error_that_names_it():
    from unlearn_saliency_amd import ops_clip
    ids = torch.tensor([[0, 5, 1000, 3]])
    with pytest.raises(ValueError, match="1000"):
        ops_clip.check_ids(ids, 1000)
    with pytest.raises(ValueError, match="-1"):
        ops_clip.check_ids(torch.tensor([[0, -1]]), 1000)
    ops_clip.check_ids(torch.tensor([[0, 999]]), 1000)
    with pytest.raises(ValueError, match="1000"):           # a host tensor is validated before any device work
        ops_clip.clip_embed(ids, torch.zeros(1000, 8), torch.zeros(4, 8))


def test_library_text_calls_counter_exists_and_is_zero():
    from unlearn_saliency_amd.SD import clip_text
    assert clip_text.LIBRARY_TEXT_CALLS and all(v == 0 for v in clip_text.LIBRARY_TEXT_CALLS.values())


# ------------------------------------------------------------------------------------------------------ the bounds' model
def test_onehot_case_has_the_properties_the_gpu_test_relies_on():
    for T in (1, 2, 15, 16, 17, 33, 64, 77):
        qkv, sel = R.onehot_case(2, 3, T)
        q, k, v = R.split_heads(qkv, 2, T, 3)
        s = q @ k.transpose(-1, -2) / 8.0
        future = 0
        for t in range(T):
            row = s[..., t, :t + 1]
            best = row.max(-1)
            assert torch.equal(best.indices, sel[..., t])
            others = row.clone()
            others.scatter_(-1, sel[..., t:t + 1], -1e30)
            assert t == 0 or bool((best.values - others.max(-1).values > 120).all())
            future += int((s[..., t, :].max(-1).values > best.values).sum())
        assert T < 8 or future >= 6 * T // 2            # for half of the queries the global best lies in the future
        o, P = R.attn_causal(qkv, 2, T, 3, 1 / 8)
        want = torch.gather(v, 2, sel[..., None].expand(-1, -1, -1, R.D)).transpose(1, 2).reshape(2 * T, 3 * R.D)
        assert torch.allclose(o, want, atol=1e-30)


# ------------------------------------------------------------------------------------------------------ command lines
def _script(name, folder=SCRIPTS):
    path = os.path.join(folder, name)
    if folder not in sys.path:
        sys.path.insert(0, folder)
    spec = importlib.util.spec_from_file_location("sd_cli_" + name.replace("-", "_").replace(".py", ""), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CLIS = [("encode_prompts.py", SCRIPTS), ("train-esd.py", SCRIPTS), ("encode_images.py", SCRIPTS),
        ("generate-images.py", os.path.join(ROOT, "unlearn_saliency_amd", "SD", "eval-scripts"))]


@pytest.mark.parametrize("name,folder", CLIS)
def test_help_names_the_tokenizer_flag(name, folder, capsys):
    mod = _script(name, folder)
    with pytest.raises(SystemExit) as e:
        getattr(mod, "full_parser", mod.build_parser)().parse_args(["--help"])       # train-esd.py: see its full_parser
    assert e.value.code == 0
    assert "--tokenizer" in capsys.readouterr().out


@pytest.mark.parametrize("name,folder,argv", [
    ("encode_prompts.py", SCRIPTS, ["--prompt", "a", "--out", "x.pt"]),
    ("train-esd.py", SCRIPTS, ["--prompt", "a", "--train_method", "xattn"]),
    ("encode_images.py", SCRIPTS, ["--manifest", "rows.csv", "--out", "x.pt"]),
    ("generate-images.py", CLIS[3][1], ["--model_name", "m", "--prompts_path", "p.csv", "--save_path", "o"])])
def test_neither_flag_error_names_the_new_flag(name, folder, argv):
    mod = _script(name, folder)
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    msg = str(e.value)
    assert "--tokenizer DIR" in msg and "vocab.json and merges.txt" in msg
    if name != "encode_prompts.py":
        assert msg.startswith("give --") and "--synthetic" in msg          # the existing sentence is still there


def test_encode_prompts_collects_csv_cells_and_esd_words(tmp_path):
    mod = _script("encode_prompts.py")
    csv_path = tmp_path / "p.csv"
    csv_path.write_text("\ufeffcase_number,prompt,evaluation_seed\n0,Image of tench,1\n1,Image of church,2\n", encoding="utf-8")
    args = mod.build_parser().parse_args(["--prompts_path", str(csv_path), "--prompt", "Van Gogh, Kelly McKernan",
                                          "--out", "x.pt", "--tokenizer", "d"])
    assert mod.collect(args) == ["", "Image of tench", "Image of church", "Van Gogh, Kelly McKernan", "Van Gogh",
                                 "Kelly McKernan"]
