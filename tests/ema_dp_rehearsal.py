"""Two-rank rehearsal of the generator weight average under data parallelism (not a pytest file: started under
torch.distributed.run by tests/test_ema_gpu.py, the pattern of tests/dp_rehearsal.py).  Each rank runs three G+D iterations of
the product on its own shard with ``StepOptions(ema=...)``; nothing is communicated for the average, so the ranks' shadows must
come out bit-identical because the all-reduced weights are.

    XMC_DIST_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
        --master-port 29512 tests/ema_dp_rehearsal.py --out ema_dp.json
Test infrastructure: builds synthetic parameters with the oracle's generator (no oracle arithmetic is the reference here)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)
import torch
import torch.distributed as dist


def main():
    if os.environ.get("XMC_DUMP_AFTER"):
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["XMC_DUMP_AFTER"]), exit=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    torch.cuda.set_device(int(os.environ["LOCAL_RANK"]) % torch.cuda.device_count())
    dist.init_process_group(os.environ.get("XMC_DIST_BACKEND", "nccl"))
    import xmc_ref as X
    import xmc_gan.train_gan as tg
    from xmc_gan_amd import ops
    from xmc_gan_amd.optim import ParamEMA
    from parity_util import DEV, build_product, setup_cfg
    ops.set_precision("fp32")
    cfg, h = setup_cfg("df_gan_damsm_nomagp.yml", **{"TRAIN.NCH": 8})
    PG, PD = X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6)
    netG, netD, optG, optD = build_product(h, PG, PD, 1e-3)
    ema = ParamEMA(netG, 0.9, 1)
    opts, st = tg.StepOptions(ema=ema), {}
    for i in range(3):
        full = X.synth_batch(h, 4 * world, seed=600 + i, words_len=cfg.TEXT.MAX_LENGTH)
        b = [full[k][rank * 4:(rank + 1) * 4].to(DEV) for k in ("imgs", "sent_embs", "words_embs", "mask", "noise")]
        tg.gan_iteration(netG, netD, optG, optD, *b, st, opts)
    torch.cuda.synchronize()
    mine = torch.cat([e.flatten().cpu() for e in ema.shadow])
    weights = torch.cat([p.detach().flatten().cpu() for p in ema.params])
    n = torch.tensor([int(ema.num_updates.item())])
    got_s, got_w, got_n = ([torch.empty_like(t) for _ in range(world)] for t in (mine, weights, n))
    dist.all_gather(got_s, mine)
    dist.all_gather(got_w, weights)
    dist.all_gather(got_n, n)
    if rank == 0:
        rep = dict(world=world, num_updates=[int(t) for t in got_n],
                   shadows_equal=all(torch.equal(got_s[0], t) for t in got_s[1:]),
                   weights_equal=all(torch.equal(got_w[0], t) for t in got_w[1:]),
                   shadow_differs_from_weights=not torch.equal(mine, weights))
        print(json.dumps(rep))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rep, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
