"""SD baselines (train_esd, gradient_ascent; K21) on the host: the numpy restatement of the K21 kernels and of the DDIM
schedule against the reference run (tests/golden/sd_baselines.npz, written by make_golden_sd_baselines.py), the two
command lines against the reference's parsers, and the train-method selections against the reference's."""
import json
import os
import re

import numpy as np
import pytest

import esd_ref_cpu as R


@pytest.fixture(scope="module")
def base(golden_dir):
    return np.load(os.path.join(golden_dir, "sd_baselines.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_schedule_equals_the_reference_tables_bit_for_bit(base):
    S = int(base["ddim_steps"])
    assert np.array_equal(_bits(R.alphas_cumprod()), _bits(base["alphas_cumprod"]))
    t = R.ddim_tables(base["alphas_cumprod"], S)
    assert np.array_equal(t["timesteps"], base["ddim_timesteps"])
    for k in ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas"):
        assert t[k].dtype == base["ddim_" + k].dtype, k
        assert np.array_equal(_bits(t[k]), _bits(base["ddim_" + k])), k


def test_package_schedule_equals_the_reference_tables_bit_for_bit(base):
    from fixtures import sd_tiny_config
    from unlearn_saliency_amd.SD.ddim import DDIMSampler
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    m = LatentDiffusionLite(sd_tiny_config())
    keys = set(m.state_dict())
    s = DDIMSampler(m).make_schedule(int(base["ddim_steps"]), 0.0)
    assert set(m.state_dict()) == keys and not any("ddim" in k or "alphas_cumprod_f32" in k for k in keys)
    assert np.array_equal(_bits(m.alphas_cumprod_f32), _bits(base["alphas_cumprod"]))
    assert np.array_equal(s.ddim_timesteps, base["ddim_timesteps"])
    for k in ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas"):
        assert np.array_equal(_bits(getattr(s, "ddim_" + k)), _bits(base["ddim_" + k])), k
    t = R.ddim_tables(base["alphas_cumprod"], int(base["ddim_steps"]))
    for index in range(int(base["ddim_steps"])):
        want = [float(v) for v in R.coefficients(t, index)]
        assert list(s.coefficients(index)) == want, index


def test_step_restatement_reproduces_the_recorded_chain(base):
    """Iteration 0 of the first ESD run (t_enc = 0: the whole chain): given the recorded batched eps of every step, the
    restated step gives the reference's x_prev bit for bit, and each x_prev is the next step's x."""
    t = R.ddim_tables(base["alphas_cumprod"], int(base["ddim_steps"]))
    xs, eps2, xp, idx = base["chain__x"], base["chain__eps2"], base["chain__x_prev"], base["chain__index"]
    assert len(xs) == int(base["esd_full_mask__steps"][0]) == int(base["ddim_steps"]) - 1
    assert list(idx) == list(range(len(xs) - 1, -1, -1))
    assert np.array_equal(_bits(xs[0]), _bits(base["esd_full_mask__start"][0]))
    for i in range(len(xs)):
        got, _ = R.ldm_ddim_step(xs[i], eps2[i], 3.0, *R.coefficients(t, int(idx[i])))
        assert np.array_equal(_bits(got), _bits(xp[i])), i
        if i + 1 < len(xs):
            assert np.array_equal(_bits(xp[i]), _bits(xs[i + 1]))
    assert np.array_equal(_bits(xp[-1]), _bits(base["esd_full_mask__z"][0]))


def test_exit_rule_as_recorded(base):
    """t_enc = 0 runs the S - 1 positions left by `timesteps[:t_start]`, t_enc = k >= 1 stops after S - k."""
    S = int(base["ddim_steps"])
    for tag in ("esd_full_mask", "esd_xattn", "esd_noxattn"):
        t_encs = base[f"{tag}__randint"][0::2]
        assert [S - 1 if k == 0 else S - int(k) for k in t_encs] == list(base[f"{tag}__steps"]), tag
    assert {0, S - 1} <= set(int(k) for k in base["esd_full_mask__randint"][0::2])


def _script(name):
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "unlearn_saliency_amd", "SD", "train-scripts")
    if d not in sys.path:
        sys.path.insert(0, d)
    spec = importlib.util.spec_from_file_location("sd_cli_" + name.replace("-", "_"), os.path.join(d, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["train-esd", "gradient_ascent"])
def test_parsers_match_the_reference(golden_dir, name):
    ref = json.load(open(os.path.join(golden_dir, "cli_sd_baselines.json")))["sd"][name]
    parser = _script(name).build_parser()
    actions = {a.dest: a for a in parser._actions if a.dest != "help"}
    assert len(ref) == (14 if name == "train-esd" else 13)
    for flag, spec in ref.items():
        assert flag in actions, f"reference flag --{flag} missing from {name}.py"
        a = actions[flag]
        assert a.required == spec.get("required", False), flag
        if "default" in spec and not a.required:
            assert a.default == spec["default"], (flag, a.default, spec["default"])
        want = {"str": str, "int": int, "float": float, "bool": bool}.get(spec.get("type"))
        if (name, flag) == ("train-esd", "lr"):
            assert a.type is float and spec["type"] == "int"   # the reference's type=int rejects its own 1e-5
        elif want is not None:
            assert a.type is want, (flag, a.type, want)
    extra = set(actions) - set(ref)
    assert extra == {"latents", "synthetic", "resident_activations", "bf16"} | ({"contexts"} if name == "train-esd" else set())


# the rules of train-esd.py:207-236 written once more, as patterns (independent of train_scripts.esd_selects)
_RULES = {
    "noxattn": lambda n: not re.search(r"^out\.|attn2|time_embed", n),
    "selfattn": lambda n: bool(re.search(r"attn1", n)),
    "xattn": lambda n: bool(re.search(r"attn2", n)),
    "full": lambda n: True,
    "notime": lambda n: not re.search(r"^out\.|time_embed", n),
    "xlayer": lambda n: bool(re.search(r"output_blocks\.(6|8)\..*attn2|attn2.*output_blocks\.(6|8)\.", n)),
    "selflayer": lambda n: bool(re.search(r"input_blocks\.(4|7)\..*attn1|attn1.*input_blocks\.(4|7)\.", n)),
}


def test_train_method_selections(golden_dir, base):
    from unlearn_saliency_amd.SD import train_scripts as TS
    assert set(TS.ESD_TRAIN_METHODS) == set(_RULES)
    # (1) on the tiny model: exactly the parameters the reference handed to its optimizer
    names = [str(n) for n in base["param_names"]]
    for method in TS.ESD_TRAIN_METHODS:
        got = [i for i, n in enumerate(names) if TS.esd_selects(n, method)]
        assert got == list(base[f"esd_selected__{method}"]), method
    # (2) on the full v1 name list: the counts per method
    full = [str(n) for n in np.load(os.path.join(golden_dir, "sd_core.npz"))["full_param_names"]]
    assert len(full) == 686
    counts = {m: sum(TS.esd_selects(n, m) for n in full) for m in TS.ESD_TRAIN_METHODS}
    assert counts == {m: sum(_RULES[m](n) for n in full) for m in _RULES}
    # 16 transformer blocks, an attention holds to_q / to_k / to_v / to_out.0.{weight, bias}; one transformer in each of
    # the named blocks; time_embed.{0, 2} and out.{0, 2} hold a weight and a bias each
    assert counts["full"] == 686 and counts["xattn"] == counts["selfattn"] == 16 * 5
    assert counts["xlayer"] == counts["selflayer"] == 2 * 5
    assert counts["notime"] == 686 - 4 - 4 and counts["noxattn"] == counts["notime"] - 80
    with pytest.raises(ValueError):
        TS.esd_selects("out.2.weight", "everything")


def test_prompt_cleaning():
    from unlearn_saliency_amd.SD import train_scripts as TS
    assert TS.esd_words("Van Gogh") == ("VanGogh", ["Van Gogh"])
    assert TS.esd_words("a, b ,c", ",") == ("a,b,c", ["a", "b", "c"])
    wp, words = TS.esd_words("i2p", ",")
    assert wp == "i2p" and words[0] == "hate" and words[-1] == "blood" and len(words) == 11
    assert len(TS.esd_words("allartist", ",")[1]) == 6 and len(TS.esd_words("artifact", ",")[1]) == 22
    assert TS.esd_name("xattn", 1e-05, None) == "compvis-esd-method_xattn-lr_1e-05"
    assert TS.esd_name("full", 1e-05, "m.pt") == "compvis-esd-mask-method_full-lr_1e-05"
    assert TS.ga_name("full", 0.1, 10, 1e-05, "m.pt") == "compvis-ga-mask-method_full-alpha_0.1-epoch_10-lr_1e-05"
