#!/usr/bin/env python
"""End-to-end use of the package the way the reference's ``main.py`` -> ``GNNTrainer`` uses its own modules
(trainer/train_gnn.py:19-120), on synthetic WSI-shaped graphs:

  graph files (io.save_graph / load_graph)  ->  GraphBatchLoader (replaces GraphDataLoader + g.to(device))  ->
  HEATNet4 (or --model HGT | GCN | GIN) + Adam + CrossEntropy via trainer.train_one_step  ->  CheckpointStore (reference file layout)  ->  io.evaluate
  (--captured-eval: trainer.CapturedSlotEval, the epoch's metrics kept on the device).

Run on one GPU:            python examples/train_synthetic.py --epochs 2          (--augment: the reference's train-time augmentation;
                           --captured-slots 3 --augment --quota --optimizer adam: captured slots sized for the draw;
                           add --type-mask: slots that also replay batches lacking a node type, DESIGN 3.29;
                           --model GCN --pooling att --captured-slots 3 --captured-eval --optimizer adam: the homogeneous baseline with the
                           attention readout, replayed over homogeneous slots, DESIGN 3.30;
                           --model GIN --captured-slots 3 --captured-eval --optimizer adam: GIN the same way, DESIGN 3.33;
                           --optimizer sgd|adagrad|adadelta|adam: the package's one-launch optimizers;
                           --captured-slots 3 --optimizer adam --cosine-lr: CosineAnnealingLR stepped once per epoch on a learning rate kept
                           as a device word, which every replay reads - nothing is recorded again)
Run data-parallel on N:    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train_synthetic.py
"""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_hgnn_amd import data, dist, io, models, parser, synthetic, trainer, transforms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--model", choices=("HEATNet4", "HGT", "GCN", "GIN"), default="HEATNet4",
                    help="HGT: the heterogeneous baseline (its layers' own dropout 0.2; --dropout is HEATNet4's and GCN's).  With --captured-slots / "
                         "--captured-eval its slots carry the per-relation-source plan, re-derived on the device behind every fill (DESIGN 3.27).  "
                         "GCN: the homogeneous baseline over graph.to_homogeneous slides with self-loops; its slots keep GraphConv's degree norms "
                         "current on the device (DESIGN 3.30).  GIN: the reference's GIN_COAD shape (2 layers, 2-layer MLPs, mean neighbours) over "
                         "the same homogeneous slides; its slots also keep the live rows and their count on the device, for its BatchNorms (DESIGN 3.33)")
    ap.add_argument("--pooling", choices=("mean", "sum", "max", "att"), default="mean",
                    help="graph_pooling_type.  att: the attention readout - in captured slots one pass over the slot's readout tables (DESIGN 3.30); "
                         "HEATNet4 and HGT apply its first gate, sized for --in-dim, to --hidden-wide states: they need --hidden == --in-dim")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--augment", action="store_true",
                    help="train on augmented graphs as the reference does (data.py:16-23: DropNode, DropEdge, NodeShuffle, FeatMask at p = 0.5)")
    ap.add_argument("--optimizer", choices=("adam", "sgd", "adagrad", "adadelta"), default=None,
                    help="step with the package's own optimizer of that name (parser.parse_optimizer(..., native=True): one HIP launch per step); "
                         "default: torch.optim.Adam")
    ap.add_argument("--captured-slots", type=int, default=0, metavar="K",
                    help="train through trainer.CapturedSlotStep over K padded batch slots by slide size (DESIGN 3.15): one captured step per slot, "
                         "replayed over every new batch that fits; needs --optimizer adam, sgd or adadelta (capturable).  With --augment the slots draw the "
                         "augmentation on the device in front of every replay (DESIGN 3.16)")
    ap.add_argument("--type-mask", action="store_true",
                    help="with --captured-slots: slots with a device-side presence table (data.BatchSlot(type_mask=True), DESIGN 3.29) - batches "
                         "that lack a node type, and augmented ones a draw can empty of one, are replayed too instead of stepped eagerly; "
                         "needs a wsi_hgnn_amd.optim optimizer (--optimizer adam, sgd or adadelta here)")
    ap.add_argument("--quota", action="store_true",
                    help="with --captured-slots and --augment: size the slots for the draw instead of for the stored slides - survivor quotas "
                         "(data.BatchSlot(quota=\"bound\"), DESIGN 3.28); the epoch line then reports in how many fills a quota bound (expected 0)")
    ap.add_argument("--cosine-lr", action="store_true",
                    help="step torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs, 5e-6) once per epoch, as the reference's one-item-per-step "
                         "baselines do.  With --captured-slots the optimizer is built with the rate as a device word (optim.lr_word, DESIGN 3.34): "
                         "the scheduler fill_s it and the captured steps follow; without, the rate is a float, as ever")
    ap.add_argument("--captured-eval", action="store_true",
                    help="evaluate through trainer.CapturedSlotEval (DESIGN 3.17): one captured forward per slot, the epoch's metrics accumulated on the "
                         "device and read back once; with --captured-slots the training metrics of the epoch come from the captured step as well")
    args = ap.parse_args(argv)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as td
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        td.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    work = args.workdir or tempfile.mkdtemp(prefix="wsi_example_")
    os.makedirs(os.path.join(work, "graphs"), exist_ok=True)
    # 1. "data set": flat safetensors graph files named like TCGA slides (label = tumour vs normal from the barcode list)
    paths, normal = [], []
    for i in range(args.graphs):
        name = f"TCGA-AA-{i:04d}-01Z-00-DX1"
        p = os.path.join(work, "graphs", name + ".safetensors")
        if rank == 0 and not os.path.exists(p):
            io.save_graph(p, synthetic.hetero_graph(args.nodes, args.in_dim, seed=100 + i, dst_mode="hub"))
        paths.append(p)
        if i % 2 == 0:
            normal.append(name[:16])
    if world > 1:
        td.barrier(device_ids=[local])
    mine = dist.shard(paths, rank, world)                                   # WSI-sharded data parallelism
    graphs = [io.load_graph(p) for p in mine]
    if args.model in ("GCN", "GIN"):                                        # the reference's homogeneous data set: one node type, self-loops added
        from wsi_hgnn_amd import graph as graph_mod
        graphs = [graph_mod.to_homogeneous(g, add_self_loop=True) for g in graphs]
    if args.pooling == "att" and args.model not in ("GCN", "GIN") and args.hidden != args.in_dim:
        raise SystemExit("--pooling att with HEATNet4 / HGT: --hidden must equal --in-dim (the first gate is sized for the input features)")
    labels = [io.label_tumour_vs_normal(p, normal) for p in mine]
    loader = data.GraphBatchLoader(graphs, labels, args.batch, dev, shuffle=True, drop_last=False, seed=611 + rank,
                                   transform=transforms.reference_train_transform() if args.augment else None)
    # evaluation sees the stored graphs: the reference augments type_ == "train" only (data.py:116-117)
    eval_loader = data.GraphBatchLoader(graphs, labels, args.batch, dev, shuffle=False, drop_last=False) if args.augment else loader

    # 2. model / optimizer / loss exactly as parser.py builds them (Adam lr 1e-5 wd 5e-3; CrossEntropyLoss)
    nd = {"0": 0, "1": 1, "2": 2}
    torch.manual_seed(611)
    hgt = args.model == "HGT"
    if hgt:
        edge_dict = {r: i for i, r in enumerate(graphs[0].canonical_etypes)}
        gnn = models.HGT(nd, edge_dict, args.in_dim, args.hidden, 2, 2, 4, use_norm=True, graph_pooling_type=args.pooling).to(dev)
    elif args.model == "GCN":
        gnn = models.GCN(args.in_dim, args.hidden, 2, 2, torch.nn.functional.relu, args.dropout, args.pooling).to(dev)
    elif args.model == "GIN":                                               # configs/COAD/GIN_COAD.yml: 2 layers, 2-layer MLPs, mean neighbours
        gnn = models.GIN(args.in_dim, args.hidden, 2, 2, 2, args.dropout, args.pooling, "mean").to(dev)
    else:
        gnn = models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, nd, args.dropout, args.pooling).to(dev)
    if args.optimizer is None:
        opt = torch.optim.Adam(gnn.parameters(), lr=1e-5, weight_decay=5e-3)
    else:
        opt = parser.parse_optimizer({"opt_method": args.optimizer, "lr": 1e-5, "weight_decay": 5e-3}, gnn, native=True)
    loss_fn = torch.nn.CrossEntropyLoss()
    bucket = dist.GradBucket.from_model(gnn) if world > 1 else None         # every parameter the architecture reaches, with used flags
    store = io.CheckpointStore(os.path.join(work, "ckpt"))

    slot_step, slot_eval, train_metrics = None, None, None
    if args.captured_eval:
        if world > 1:
            raise SystemExit("--captured-eval: single process")
        from wsi_hgnn_amd.metrics import EpochMetrics
        slot_eval = trainer.CapturedSlotEval(gnn, [data.BatchSlot(eval_loader, per_relation_src=hgt)])
        if args.captured_slots:
            train_metrics = EpochMetrics(2, len(graphs), dev)
    if args.captured_slots:
        if world > 1 or args.optimizer not in ("adam", "sgd", "adadelta"):
            raise SystemExit("--captured-slots: single process and --optimizer adam | sgd | adadelta")
        if args.cosine_lr:                                                   # the rate a device word (and Adam's count on the device)
            opt = parser.parse_optimizer({"opt_method": args.optimizer, "lr": 1e-5, "weight_decay": 5e-3}, gnn, native=True, device_lr=True)
        elif args.optimizer == "adam":
            from wsi_hgnn_amd import optim
            opt = optim.Adam(gnn.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)         # the step count on the device
        # slot k holds any `batch` slides out of the smallest (k + 1) / K of the data set; the last one every batch
        its, K = sorted(loader.items, key=lambda it: sum(it.num_nodes)), args.captured_slots
        top = lambda xs: sum(sorted(xs, reverse=True)[:args.batch])
        nodes_of, edges_of = (lambda it: it.num_nodes), (lambda it: it.pieces.ecount)
        if args.quota:
            if not args.augment:
                raise SystemExit("--quota: quotas limit the survivors of a draw; add --augment")
            # the same classes over the slides' quotas: what a draw leaves of a slide at most (it binds with probability 2 ** -32 per table)
            spec = data.slot_augment_spec(loader.transform)
            dst = [its[0].ntypes.index(r[2]) for r in its[0].rels]
            nodes_of = lambda it: data.slot_quota_bound(it, spec)[0]
            edges_of = lambda it: [sum(q for q, d in zip(data.slot_quota_bound(it, spec)[1], dst) if d == t) for t in range(len(it.num_nodes))]
        caps = []
        for k in range(K):
            part = its[:max(args.batch, (len(its) * (k + 1) + K - 1) // K)]
            caps.append(([top([nodes_of(it)[t] for it in part]) + 1 for t in range(len(its[0].num_nodes))], [top([edges_of(it)[t] for it in part]) for t in range(len(its[0].num_nodes))], args.batch))
        gnn.train()
        slot_step = trainer.CapturedSlotStep(gnn, opt, loss_fn, [data.BatchSlot(loader, c, per_relation_src=hgt, quota="bound" if args.quota else None,
                                                                                    type_mask=args.type_mask) for c in caps],
                                             metrics=train_metrics)

    # the reference's baselines: CosineAnnealingLR(optimizer, num_epochs, 5e-6), stepped once per epoch.  On a word it ends in a fill_, which
    # the captured steps read at their next replay; on a float it assigns group["lr"], which an eager step reads
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, args.epochs, 5e-6) if args.cosine_lr else None

    # 3. epochs
    for epoch in range(args.epochs):
        gnn.train()
        tot, n = 0.0, 0
        if train_metrics is not None:
            train_metrics.reset()
        if slot_step is not None:
            order = torch.randperm(len(graphs), generator=loader.gen).tolist()
            losses = [slot_step.step(order[i:i + args.batch])[0].clone() for i in range(0, len(order), args.batch)]     # no host sync inside the epoch
            tot, n = float(torch.stack(losses).sum().item()), len(losses)
        for G, y in (loader if slot_step is None else ()):
            loss, acc, *_ = trainer.train_one_step(gnn, opt, loss_fn, G, y, dev, bucket=bucket, sync=True)
            tot, n = tot + loss, n + 1
        if scheduler is not None:
            scheduler.step()
        gnn.eval()
        metrics = io.evaluate(gnn, eval_loader) if slot_eval is None else slot_eval.evaluate()
        if rank == 0:
            print(f"epoch {epoch}: train loss {tot / max(n, 1):.4f}  eval {metrics}")
            if slot_step is not None:
                print(f"epoch {epoch}: {slot_step.replays} steps replayed, {slot_step.eager_steps} stepped eagerly so far")
            if scheduler is not None:
                print(f"epoch {epoch}: lr for the next epoch {float(opt.param_groups[0]['lr']):.3e}" + (" (a device word)" if slot_step is not None else ""))
            if slot_step is not None and args.quota:                            # one read-back per slot and epoch
                print(f"epoch {epoch}: fills truncated by a quota so far {slot_step.overflows()} of {slot_step.replays} replayed steps")
            if train_metrics is not None:                                       # train_gnn.py:104-108, one read-back per epoch
                print(f"epoch {epoch}: train metrics {train_metrics.compute()}")
            store.save_model(gnn.state_dict(), version=epoch + 1, stats={"epoch": epoch, "loss": tot / max(n, 1), **metrics})
    if rank == 0:
        sd = store.load_model()
        gnn.load_state_dict(sd)
        print("checkpoint reloaded from", store.model_file(store.load_version()))
    if world > 1:
        td.destroy_process_group()
    return work


if __name__ == "__main__":
    main()
