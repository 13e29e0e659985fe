"""The CLIP text encoder of SD v1 (vocabulary 49,408, width 768, 12 layers, 12 heads, MLP 3,072, 77 tokens) on one GPU:
TextPlan (K29 + the K15 GEMM) beside the same module on library ops, the causal attention kernel alone, and where the
plan's time goes.

  encode     seconds per pass of TextPlan.forward and of ClipTextLite.forward under torch.no_grad() at B = 2 and B = 8,
             alternated in ONE process, device events around each pass, median and range over `--reps`
  attention  salun_attn_causal_f32 at B H = 24 and 96, T = 77, beside fp32 F.scaled_dot_product_attention(is_causal=True)
             on [B, H, T, 64] tensors (the library reads contiguous heads; the kernel reads the fused qkv buffer in place)
  launches   kernel calls of one pass, and each kernel's share: its isolated time at the pass's shapes x its count over
             the pass's time (isolated kernels run back to back, so shares that sum to less than 1 are launch gaps)

    python tools/clip_text_bench.py [--reps 9] [--group 5] [--out profiles/clip_text_bench.json]

Weights are seeded random numbers (timing does not depend on them).  Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_times(run, reps, group):
    import torch
    for fn in run.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():                 # alternated: all see the same clocks and the same neighbours
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / group)
    return {k: sorted(v) for k, v in times.items()}


def _stats(t, scale=1e6, unit="us"):
    return {f"{unit}_median": round(statistics.median(t) * scale, 3), f"{unit}_min": round(t[0] * scale, 3),
            f"{unit}_max": round(t[-1] * scale, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--group", type=int, default=5, help="back-to-back calls per timed window of a single kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_text_bench.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("clip_text_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd import gemm, ops_clip
    from unlearn_saliency_amd.SD import clip_text

    torch.manual_seed(0)
    with torch.device("cuda"):
        model = clip_text.ClipTextLite.v1()
    model.requires_grad_(False).eval()
    plan = clip_text.TextPlan(model)
    cfg = model.config
    T, W, H, Fm = cfg["positions"], cfg["width"], cfg["heads"], cfg["mlp"]

    enc = []
    for B in (2, 8):
        ids = torch.randint(0, cfg["vocab_size"], (B, T))
        d_ids = ids.cuda()

        def lib():
            with torch.no_grad():
                return model(ids.cuda())          # both sides start from the tokenizer's host ids

        own, ref = plan.forward(ids), lib()
        agree = float((own - ref).abs().max() / ref.abs().max())
        t = _event_times({"plan": lambda: plan.forward(ids), "library": lib}, a.reps, 1)
        enc.append({"batch": B, "rows": B * T, "plan": _stats(t["plan"], 1e3, "ms"), "library": _stats(t["library"], 1e3, "ms"),
                    "library_over_plan": round(statistics.median(t["library"]) / statistics.median(t["plan"]), 3),
                    "max_difference_over_max": agree, "launches": plan.launches,
                    "LIBRARY_TEXT_CALLS": dict(clip_text.LIBRARY_TEXT_CALLS)})
        if B == 2:                                # where the time goes, at the shapes of this pass
            M = B * T
            lyr = model.text_model.encoder.layers[0]
            wqkv, bqkv = plan._qkv[0]
            x, h, o = (torch.randn(M, W, device="cuda") for _ in range(3))
            qkv, u = torch.randn(M, 3 * W, device="cuda"), torch.randn(M, Fm, device="cuda")
            tm = model.text_model
            parts = {
                "embed": (1, lambda: ops_clip.clip_embed(d_ids, tm.embeddings.token_embedding.weight,
                                                         tm.embeddings.position_embedding.weight, out=x)),
                "layer_norm": (2 * cfg["layers"] + 1,
                               lambda: ops_clip.ln_f32_forward(x, lyr.layer_norm1.weight, lyr.layer_norm1.bias, 1e-5, out=h)),
                "qkv_gemm": (cfg["layers"], lambda: gemm.mm_nt(h, wqkv, out=qkv, bias=bqkv)),
                "attention": (cfg["layers"], lambda: ops_clip.attn_causal_f32(qkv, B, T, H, 0.125, out=o)),
                "out_proj_gemm": (cfg["layers"], lambda: gemm.mm_nt(o, lyr.self_attn.out_proj.weight, out=x,
                                                                    bias=lyr.self_attn.out_proj.bias, accumulate=True)),
                "fc1_gemm": (cfg["layers"], lambda: gemm.mm_nt(h, lyr.mlp.fc1.weight, out=u, bias=lyr.mlp.fc1.bias)),
                "quick_gelu": (cfg["layers"], lambda: ops_clip.quick_gelu_(u)),
                "fc2_gemm": (cfg["layers"], lambda: gemm.mm_nt(u, lyr.mlp.fc2.weight, out=x, bias=lyr.mlp.fc2.bias,
                                                               accumulate=True)),
            }
            tk = _event_times({k: fn for k, (_, fn) in parts.items()}, a.reps, a.group)
            total = statistics.median(t["plan"])
            shares = {k: dict(_stats(tk[k]), count=parts[k][0],
                              share_of_plan=round(parts[k][0] * statistics.median(tk[k]) / total, 4)) for k in parts}
            enc[-1]["kernels"] = shares
            enc[-1]["kernels_share_sum"] = round(sum(v["share_of_plan"] for v in shares.values()), 4)

    att = []
    for BH in (24, 96):
        B = BH // H
        qkv = torch.randn(B * T, 3 * W, device="cuda")
        o = torch.empty(B * T, W, device="cuda")
        q, k, v = (qkv.view(B, T, 3, H, 64)[:, :, i].transpose(1, 2).contiguous() for i in range(3))
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B * T, W)
        agree = float((ops_clip.attn_causal_f32(qkv, B, T, H, 0.125) - ref).abs().max())
        t = _event_times({"k29": lambda: ops_clip.attn_causal_f32(qkv, B, T, H, 0.125, out=o),
                          "library": lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True)}, a.reps, a.group)
        att.append({"BH": BH, "T": T, "k29": _stats(t["k29"]), "library": _stats(t["library"]),
                    "library_over_k29": round(statistics.median(t["library"]) / statistics.median(t["k29"]), 3),
                    "max_difference": agree})

    line = json.dumps({"workload": "sd_clip_text_encoder", "config": cfg, "reps": a.reps, "group": a.group, "encode": enc,
                       "attention": att})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
