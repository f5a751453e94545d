"""Entry point of the Shelgon (VQ sentence autoencoder) run on MI355X -- counterpart of models/shelgon3/main.py:40-187.

    PYTHONPATH=kindergarten-vq-vae_amd python3 kindergarten-vq-vae_amd/models/shelgon3/main.py             # 1 GPU
    PYTHONPATH=kindergarten-vq-vae_amd python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 kindergarten-vq-vae_amd/models/shelgon3/main.py                            # 8 GPUs, RCCL

Same wiring as the reference: dataset -> 60/20/20 split with Generator(seed=DS_GEN_SEED) -> loaders ->
VectorQuantizer -> Shelgon -> set_mode -> tokenizer -> Adam + MultiStepLR -> run dir + run_conf.json -> train ->
reload best-val checkpoint -> test -> decoded sentences to feather.  Multi-GPU is plain data parallel
(kvq.ddp.GradSync); `model.compile()` of the reference (main.py:83) has no counterpart: the fused kernels are
hand written, there is no tracing compiler in this build.
"""
import json
import os
import sys
from datetime import datetime

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))      # package root (common/, kvq/, models/, dsentences/)
sys.path.insert(0, _HERE)

from config import *  # noqa: E402,F401,F403

import torch  # noqa: E402
from torch.optim.adam import Adam  # noqa: E402
from torch.optim.lr_scheduler import MultiStepLR  # noqa: E402
from torch.utils.data import DataLoader, random_split  # noqa: E402
from torch.utils.data.distributed import DistributedSampler  # noqa: E402

from common.consts import *  # noqa: E402,F401,F403
from dsentences.dataset import dSentencesDataset  # noqa: E402
from dsentences.synthetic import write_corpus  # noqa: E402
from dsentences.token_cache import cache_of_split  # noqa: E402
from kvq import ddp  # noqa: E402
from kvq._ffi import KvqError  # noqa: E402
from kvq.engine import TrainEngine  # noqa: E402
from kvq.free_running import FreeRunningEval, check_free_running_config, label_cardinalities  # noqa: E402
from kvq.runlog import init_run  # noqa: E402
from kvq.tokenizer import load_tokenizer  # noqa: E402
from kvq.train_state import config_differences, load_optimizer, load_train_state, resolve_path  # noqa: E402
from models.shelgon3.Shelgon import Shelgon  # noqa: E402
from models.shelgon3.Trainer import test, train  # noqa: E402
from models.shelgon3.GumbelQuantizer import GumbelQuantizer  # noqa: E402
from models.shelgon3.MultiVectorQuantizer import MultiVectorQuantizer  # noqa: E402
from models.shelgon3.VectorQuantizer import VectorQuantizer  # noqa: E402


def main():
    # FREE_RUNNING_EVAL: refused here, before anything is set up, when the configuration cannot run it
    check_free_running_config(FREE_RUNNING_EVAL, FREE_RUNNING_EVAL_VAL, FREE_RUNNING_EVAL_BEAMS, DECODER_NEXT_TOKEN, USE_ENGINE,
                              int(os.environ.get("WORLD_SIZE", "1") or 1))
    rank, local_rank, world = ddp.init_distributed()
    is_main = rank == 0
    if not torch.cuda.is_available():
        raise SystemExit("models/shelgon3/main.py needs an MI355X: the VQ / loss kernels have no CPU fallback")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    if not os.path.exists(SENTENCES_PATH):          # the corpus is git-ignored upstream and absent offline
        if is_main:
            write_corpus(os.path.dirname(SENTENCES_PATH), SYNTHETIC_SENTENCES, seed=DS_GEN_SEED)
        if world > 1:
            torch.distributed.barrier()
    ds = dSentencesDataset(SENTENCES_PATH, LATENT_CLASSES_LABELS_PATH, LATENT_CLASSES_ONE_HOT_PATH)
    ds_train_len = int(len(ds) * TRAIN_SPLIT_PCT)
    ds_val_len = int(len(ds) * VAL_SPLIT_PCT)
    ds_test_len = len(ds) - ds_train_len - ds_val_len
    ds_gen = torch.Generator()
    ds_gen.manual_seed(DS_GEN_SEED)
    ds_train, ds_val, ds_test = random_split(ds, (ds_train_len, ds_val_len, ds_test_len), ds_gen)

    def loader(split, shuffle):
        sampler = DistributedSampler(split, world, rank, shuffle=shuffle, drop_last=True) if world > 1 else None
        return DataLoader(split, batch_size=BATCH_SIZE, num_workers=NUM_WORKERS, pin_memory=PIN_MEMORY,
                          shuffle=shuffle and sampler is None, sampler=sampler, drop_last=world > 1)
    dl_train, dl_val, dl_test = loader(ds_train, True), loader(ds_val, False), loader(ds_test, False)

    if VQ_MODE == "VectorQuantizer":
        init = torch.load(VQ_CODEBOOK_INIT_VALUES_PATH)["codebook_init_values"] if VQ_CODEBOOK_INIT_VALUES_PATH else None
        vector_quantizer = VectorQuantizer(n_e=VQ_N_E, e_dim=VQ_E_DIM, beta=VQ_BETA, vq_codebook_init_values=init,
                                           ema_decay=VQ_EMA_DECAY, revive_after=VQ_REVIVE_AFTER)
        vector_quantizer.materialize_min_encodings = False          # the model drops min_encodings (Shelgon.py:58)
    elif VQ_MODE == "MultiVectorQuantizer":                         # extension (BASELINE.json configs[4]), off by default
        vector_quantizer = MultiVectorQuantizer(n_factors=VQ_N_FACTORS, n_e=VQ_N_E, e_dim=VQ_E_DIM, beta=VQ_BETA,
                                                ema_decay=VQ_EMA_DECAY, revive_after=VQ_REVIVE_AFTER)
    elif VQ_MODE == "GumbelQuantizer":                              # main.py:68-73
        vector_quantizer = GumbelQuantizer(enc_out_size=ENC_OUT_SIZE, n_embed=VQ_N_E, embedding_dim=VQ_E_DIM,
                                           temperature=VQ_TEMPERATURE, kl_div_scale=VQ_KL_DIV_SCALE,
                                           straight_through=VQ_STRAIGHT_THROUGH)
    else:
        raise ValueError(f"{VQ_MODE} vector quantizer mode NOT supported. Supported modalities: VectorQuantizer, GumbelQuantizer")

    torch.manual_seed(0)                                          # same init on every rank
    model = Shelgon(encoder_model_name=ENCODER_MODEL_NAME, vector_quantizer=vector_quantizer,
                    decoder_model_name=DECODER_MODEL_NAME, from_pretrained_bagon=FROM_PRETRAINED_BAGON,
                    cross_attn_make_trainable=CROSS_ATTN_MAKE_TRAINABLE,
                    compute_dtype=getattr(torch, COMPUTE_DTYPE)).to(device)
    model.set_mode(MODEL_MODE)
    ddp.broadcast_parameters(model)
    if is_main:
        model.model_params_summary_print()

    tokenizer = load_tokenizer(TOKENIZER_NAME)
    if TOKEN_CACHE:
        # every split tokenised once and kept in HBM; a batch is an index_select on the device (no per-step tokenizer / H2D)
        caches = [cache_of_split(sp, tokenizer, TOKENIZED_SENTENCE_MAX_LENGTH, TOKENIZER_ADD_SPECIAL_TOKENS, device, keep_labels=FREE_RUNNING_EVAL)
                  for sp in (ds_train, ds_val, ds_test)]
        dl_train = caches[0].loader(BATCH_SIZE, True, seed=DS_GEN_SEED, rank=rank, world=world)
        dl_val = caches[1].loader(BATCH_SIZE, False, rank=rank, world=world)
        dl_test = caches[2].loader(BATCH_SIZE, False, rank=rank, world=world)
    opt = Adam(params=[p for p in model.parameters()], lr=LR, weight_decay=WEIGHT_DECAY, amsgrad=AMSGRAD, fused=True)
    lr_sched = MultiStepLR(optimizer=opt, milestones=MILESTONES, gamma=GAMMA) if LR_SCHEDULER == "MultiStepLR" else None
    engine = grad_sync = None
    if USE_ENGINE and TrainEngine.supports(model, TOKENIZED_SENTENCE_MAX_LENGTH):
        # explicit forward/backward schedule on flat buffers (kvq/engine.py): owns Adam, the scheduler tick and the
        # RCCL gradient exchange; `opt` above is then only the reference-shaped handle recorded in run_conf.json
        engine = TrainEngine(model, lr=LR, weight_decay=WEIGHT_DECAY, amsgrad=AMSGRAD,
                             milestones=MILESTONES if LR_SCHEDULER == "MultiStepLR" else None, gamma=GAMMA,
                             loss_recon_scale=LOSS_RECON_RESCALE_FACTOR * LOSS_RECON_WEIGHT,
                             loss_vq_scale=LOSS_VQ_RESCALE_FACTOR * LOSS_VQ_WEIGHT, bucket_mib=GRAD_BUCKET_MIB,
                             fp8_forward=FP8_FORWARD if FP8_FORWARD else None,       # (None: the KVQ_FP8 environment switch decides)
                             fp8_backward=FP8_BACKWARD if FP8_BACKWARD else None,     # (None: KVQ_FP8_BACKWARD)
                             max_grad_norm=MAX_GRAD_NORM,                             # (None: off, or KVQ_MAX_GRAD_NORM)
                             grad_accum=GRAD_ACCUM_STEPS,                             # (1: off; the configuration has read KVQ_GRAD_ACCUM)
                             weight_ema=WEIGHT_EMA_DECAY,                             # (None: off; the configuration has read KVQ_WEIGHT_EMA)
                             loss_ignore_pad=LOSS_IGNORE_PAD,                         # (the configuration has read KVQ_LOSS_IGNORE_PAD)
                             param_groups=PARAM_GROUPS, decoupled_weight_decay=DECOUPLED_WEIGHT_DECAY,      # (the
                             lr_warmup_steps=LR_WARMUP_STEPS, lr_decay=LR_DECAY,                            # configuration has read their
                             lr_total_steps=LR_TOTAL_STEPS, lr_min_ratio=LR_MIN_RATIO)                      # KVQ_* variables)
        if TOKEN_CACHE:
            for c in caches:          # the packed sort files the MODEL's padding row under -1 (not the tokenizer's pad id)
                c.packed_pad_id = engine.pad_idx
    elif world > 1:
        grad_sync = ddp.GradSync(model.parameters(), bucket_mib=GRAD_BUCKET_MIB)
    if engine is None and GRAD_ACCUM_STEPS > 1:      # the autograd path steps its optimiser per batch: no silent batch of another size
        raise SystemExit("GRAD_ACCUM_STEPS > 1 (KVQ_GRAD_ACCUM) needs the engine (USE_ENGINE and a model shape it supports)")
    if DECODER_NEXT_TOKEN:      # next-token training: the trainer's step shifts the decoder input by this start id
        if engine is None:
            raise SystemExit("DECODER_NEXT_TOKEN needs the engine (USE_ENGINE and a model shape it supports)")
        from kvq.tokenizer import CLS
        start_id = getattr(tokenizer, "cls_token_id", None)
        model.decoder_next_token_start_id = int(CLS if start_id is None else start_id)
    free_running = None
    if FREE_RUNNING_EVAL:       # free-running reconstruction metrics in the test stage (and validation): DESIGN.md section 5l
        if engine is None:
            raise ValueError("FREE_RUNNING_EVAL needs the engine (USE_ENGINE and a model shape it supports)")
        from kvq.tokenizer import SEP
        eos_id = getattr(tokenizer, "sep_token_id", None)
        free_running = FreeRunningEval(engine, model.decoder_next_token_start_id,
                                       eos_id=int(SEP if eos_id is None else eos_id) if TOKENIZER_ADD_SPECIAL_TOKENS else None,
                                       num_beams=FREE_RUNNING_EVAL_BEAMS, validation=FREE_RUNNING_EVAL_VAL,
                                       cardinalities=label_cardinalities(ds.latent_classes_labels))
    if engine is None and LOSS_IGNORE_PAD:      # the autograd path: forward_loss hands the pad id to fused_cross_entropy(ignore_index=...)
        model.loss_ignore_index = model.decoder.bert.embeddings.word_embeddings.padding_idx
        if model.loss_ignore_index is None:
            raise SystemExit("LOSS_IGNORE_PAD (KVQ_LOSS_IGNORE_PAD) needs word embeddings with a padding_idx")
    if engine is None and (PARAM_GROUPS is not None or DECOUPLED_WEIGHT_DECAY or LR_WARMUP_STEPS > 0 or LR_DECAY is not None):
        # groups, the decoupled decay and the schedule live in the engine's Adam / step-state kernels: no silent run under `opt`'s rule
        raise SystemExit("PARAM_GROUPS / DECOUPLED_WEIGHT_DECAY / LR_WARMUP_STEPS / LR_DECAY need the engine (USE_ENGINE and a model shape it supports)")
    if engine is None and WEIGHT_EMA_DECAY is not None:      # the average is built inside the engine's step: no silent run without it
        raise SystemExit("WEIGHT_EMA_DECAY (KVQ_WEIGHT_EMA) needs the engine (USE_ENGINE and a model shape it supports)")

    # RESUME_FROM: continue a run from its training-state file (kvq/train_state.py).  Every rank reads the SAME
    # file and takes the same decisions from it, so a refusal stops all of them; a rank that cannot read it stops all of them too.
    state_config = dict(get_config(), ds_gen_seed=DS_GEN_SEED, world_size=world)      # + what decides an epoch's batches besides config.py
    resume = None
    if RESUME_FROM is not None:
        state_file = resolve_path(RESUME_FROM, "shelgon_train_state_last.pth")
        if not ddp.readable_everywhere(state_file):
            raise SystemExit(f"RESUME_FROM: {state_file} cannot be read on every rank (all ranks read one file: a shared filesystem)")
        resume = load_train_state(state_file, map_location="cpu")
        diff = config_differences(resume["config"], state_config)
        if diff:
            raise SystemExit("RESUME_FROM: the stored run was configured differently -- " + "; ".join(diff))
        if (engine is not None) != ("engine" in resume):
            raise SystemExit(f"RESUME_FROM: the stored run trained {'on the engine' if 'engine' in resume else 'on the autograd path'}, "
                             f"this one is set up for the other (USE_ENGINE)")
        model.load_state_dict(resume["model_state_dict"])
        if engine is not None:
            try:
                engine.load_state_dict(resume["engine"])
            except KvqError as e:
                raise SystemExit(f"RESUME_FROM: {e}") from None
        else:
            load_optimizer(resume, opt, lr_sched)

    console = prg = None
    if is_main:
        from rich.console import Console
        from rich.progress import BarColumn, MofNCompleteColumn, Progress, TextColumn, TimeElapsedColumn, TimeRemainingColumn
        console = Console()
        prg = Progress(TextColumn("[progress.description]{task.description}"), BarColumn(), MofNCompleteColumn(),
                       TimeElapsedColumn(), TimeRemainingColumn(), TextColumn("[bold #5B4328]{task.speed} it/s"), console=console)

    run_id = ddp.same_everywhere(datetime.now().strftime(RUN_ID_TIMESTAMP_FORMAT))     # one run directory for all ranks
    run_path = f"{RUNS_DIR}/{run_id}"
    if resume is not None:                    # the resumed run goes on in the stored run's directory, under its id
        run_path = os.path.dirname(os.path.abspath(state_file))
        run_id = resume["config"].get("run_id") or os.path.basename(run_path)
    state_config["run_id"] = run_id
    run_conf = get_config()
    run_conf.update({"n_params": model.model_params_summary_dict(), "optimizer": str(opt), "run_id": run_id, "world_size": world,
                     "grad_accum": engine.grad_accum if engine is not None else 1,
                     "max_grad_norm": engine.max_grad_norm if engine is not None else None,      # what the step really runs with
                     "weight_ema": engine.weight_ema if engine is not None else None,
                     "loss_ignore_pad": engine.loss_ignore_pad if engine is not None else model.loss_ignore_index is not None,
                     "vq_revive_after": engine.revive_after if engine is not None else getattr(vector_quantizer, "revive_after", None)})
    if is_main:
        os.makedirs(run_path, exist_ok=True)
        console.print(f"Run ID: [bold {COLOR_RUN_ID}]{run_id}\n")
        if resume is None:                    # (a resumed run leaves the stored run's run_conf.json as it is)
            with open(f"{run_path}/run_conf.json", "w") as fp:
                json.dump(run_conf, fp)
    os.environ["WANDB_SILENT"] = WANDB_SILENT
    wandb_run = init_run(WANDB_PROJECT_NAME, WANDB_GROUP, WANDB_JOB_TYPE, run_conf, WANDB_MODE if is_main else "disabled",
                         run_path if is_main else None)

    weights = dict(loss_recon_rescale_factor=LOSS_RECON_RESCALE_FACTOR, loss_recon_weight=LOSS_RECON_WEIGHT,
                   loss_vq_rescale_factor=LOSS_VQ_RESCALE_FACTOR, loss_vq_weight=LOSS_VQ_WEIGHT,
                   loss_perp_rescale_factor=LOSS_PERP_RESCALE_FACTOR, loss_perp_weight=LOSS_PERP_WEIGHT)
    n_batches_train = int(len(dl_train) * LIM_BATCHES_TRAIN_PCT)
    n_batches_val = int(len(dl_val) * LIM_BATCHES_VAL_PCT)
    decoded_sentences = []
    if resume is not None:
        wandb_run.log({"resumed_after_epoch": resume["trainer"]["epoch"]})
    train(prg=prg, console=console, device=device, dl_train=dl_train, dl_val=dl_val, n_batches_train=n_batches_train,
          n_batches_val=n_batches_val, model=model, tokenizer=tokenizer, tokenizer_add_special_tokens=TOKENIZER_ADD_SPECIAL_TOKENS,
          n_epochs_to_decode_after=N_EPOCHS_TO_DECODE_AFTER, decoded_sentences=decoded_sentences, opt=opt, lr_sched=lr_sched,
          n_epochs=N_EPOCHS, vocab_size=VOCAB_SIZE, wandb_run=wandb_run, run_path=run_path, export_checkpoint=EXPORT_CHECKPOINT,
          max_length=TOKENIZED_SENTENCE_MAX_LENGTH, grad_sync=grad_sync, is_main=is_main, engine=engine,
          train_state_path=f"{run_path}/shelgon_train_state_last.pth" if EXPORT_TRAIN_STATE else None,
          train_state_every=TRAIN_STATE_EVERY_EPOCHS, resume=resume, train_state_config=state_config,
          weight_ema_eval=WEIGHT_EMA_EVAL, free_running=free_running, **weights)

    # The test stage runs on EVERY rank (each on its shard of the test split): test() ends in the stage's all-reduce of the
    # statistics (Trainer._sum_over_ranks), a collective every rank has to enter.  Rank 0 wrote the checkpoint; agree() puts a
    # barrier behind that write and hands every rank rank 0's answer to "is there a best checkpoint".
    best = f"{run_path}/shelgon_ckpt_loss_recon_val_best.pth"
    if ddp.agree(EXPORT_CHECKPOINT and os.path.exists(best)):
        model.load_state_dict(torch.load(best, map_location=device)["model_state_dict"])
        if engine is not None:
            engine.sync_from_model()
        n_batches_test = int(len(dl_test) * LIM_BATCHES_TEST_PCT)
        test(prg=prg, console=console, device=device, dl_test=dl_test, n_batches_test=n_batches_test, model=model,
             tokenizer=tokenizer, tokenizer_add_special_tokens=TOKENIZER_ADD_SPECIAL_TOKENS, decoded_sentences=decoded_sentences,
             vocab_size=VOCAB_SIZE, epoch=N_EPOCHS, wandb_run=wandb_run, max_length=TOKENIZED_SENTENCE_MAX_LENGTH, engine=engine,
             # weight_ema: with WEIGHT_EMA_EVAL the checkpoint just loaded was written under the average and HOLDS the averaged
             # weights that were scored -- they are tested as they are (the scope would put the last epoch's average in their place)
             weight_ema_eval=False, free_running=free_running, **weights)
        if free_running is not None and is_main:
            free_running.write_report(f"{run_path}/reconstruction_by_factor.md", "test")
    decoded_sentences = ddp.gather_lists(decoded_sentences)      # every rank decoded its own shard: rank 0 writes them all
    if is_main:
        if prg is not None:
            prg.stop()
        import pandas as pd
        try:
            pd.DataFrame(decoded_sentences).to_feather(f"{run_path}/decoded_sentences.feather")      # main.py:183-184
        except ImportError as e:          # feather needs pyarrow
            print(f"[main] feather export unavailable ({e}); writing CSV instead")
            pd.DataFrame(decoded_sentences).to_csv(f"{run_path}/decoded_sentences.csv", index=False)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
