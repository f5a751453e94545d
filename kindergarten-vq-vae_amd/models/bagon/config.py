"""Run configuration of the Bagon (plain BERT->BERT autoencoder) entry point: UPPER_CASE constants + get_config().

Counterpart of the git-ignored models/bagon/config.py the reference imports with `from config import *`
(models/bagon/main.py:1,102); constant names reconstructed from their use in main.py / Trainer.py.
Override any of them from the environment with KVQ_<NAME>=<python literal>."""
import ast as _ast
import os as _os

DATASET_PATH = "./data/dSentences/dSentences_sentences_clean.npy"
LATENT_CLASSES_LABELS_PATH = "./data/dSentences/dSentences_latent_classes_labels_clean.npy"
LATENT_CLASSES_ONE_HOT_PATH = "./data/dSentences/dSentences_latent_classes_one_hot_clean.npy"
SYNTHETIC_SENTENCES = 65536
TRAIN_SPLIT_PCT = 0.6
VAL_SPLIT_PCT = 0.2
BATCH_SIZE = 256
NUM_WORKERS = 0
PIN_MEMORY = True
TOKEN_CACHE = True              # tokenise every split once, keep it in HBM, batches = device index_select (dsentences/token_cache.py)

ENCODER_MODEL_NAME = "bert-base-uncased"
DECODER_MODEL_NAME = "bert-base-uncased"
CROSS_ATTN_MAKE_TRAINABLE = True
MODEL_MODE = "full"
COMPUTE_DTYPE = "bfloat16"
TOKENIZER_NAME_ENCODER = "bert-base-uncased"
TOKENIZER_NAME_DECODER = "bert-base-uncased"
TOKENIZER_ADD_SPECIAL_TOKENS = False
TOKENIZED_SENTENCE_MAX_LENGTH = 32
ENCODER_PERTURB_TRAIN_PCT = 0.0
ENCODER_PERTURB_VAL_PCT = 0.0
ENCODER_PERTURB_TEST_PCT = 0.0
DECODER_PERTURB_TRAIN_PCT = 0.0
DECODER_PERTURB_VAL_PCT = 0.0
DECODER_PERTURB_TEST_PCT = 0.0
VOCAB_SIZE_ENCODER = 30522
VOCAB_SIZE_DECODER = 30522

LR = 1e-4
WEIGHT_DECAY = 0.0
AMSGRAD = False
LR_SCHEDULER = "MultiStepLR"
MILESTONES = [10000, 20000]
GAMMA = 0.1
N_EPOCHS = 1
N_EPOCHS_TO_DECODE_AFTER = 1
LIM_BATCHES_TRAIN_PCT = 1.0
LIM_BATCHES_VAL_PCT = 1.0
LIM_BATCHES_TEST_PCT = 1.0
GRAD_BUCKET_MIB = 64
USE_ENGINE = True               # kvq.engine.TrainEngine (explicit fwd/bwd on flat buffers, own HIP kernels) when the model shape allows
FP8_FORWARD = False             # extension (BASELINE.json configs[4]): forward GEMMs on the fp8 matrix cores -- False | True | "wide" | "all"
FP8_BACKWARD = False            # option on top of FP8_FORWARD: input-gradient GEMMs on fp8 (e5m2 gradients, transposed e4m3 weights); DESIGN.md section 5
MAX_GRAD_NORM = None            # None (off) | float > 0 | float("inf"): the engine step clips its gradient by the global norm and skips non-finite steps (inf: measure and skip only); KVQ_MAX_GRAD_NORM; DESIGN.md section 5b
GRAD_ACCUM_STEPS = 1            # int >= 1: train_step calls (micro-batches) per optimiser step -- the engine sums their gradients in f32 and Adam reads the mean; MILESTONES, engine.step_count and the bias corrections count OPTIMISER steps, perf/train_steps counts calls; KVQ_GRAD_ACCUM; DESIGN.md section 5d
WEIGHT_EMA_DECAY = None       # None (off) | float in (0, 1): the engine keeps an f32 moving average of the trained weights, updated behind Adam inside the step (the decay warms up as min(decay, (1 + t) / (10 + t))); KVQ_WEIGHT_EMA; DESIGN.md section 5f
WEIGHT_EMA_EVAL = True         # with WEIGHT_EMA_DECAY: validation, the best-val checkpoints and the test stage run under the average (False: the average is kept and saved with the training state, evaluation reads the live weights)
LOSS_IGNORE_PAD = False        # False | True: the engine step takes the reconstruction loss, the accuracy and the per-sentence accuracy over the tokens whose target is not the pad id (F.cross_entropy's ignore_index) instead of over all B*S positions; KVQ_LOSS_IGNORE_PAD; DESIGN.md section 5g
DECODER_NEXT_TOKEN = False          # False | True: next-token training -- the decoder reads shift_right(ids, [CLS]) and its logits at t are scored against ids[t] (target_ids), instead of the reference's unshifted loss, under which a causal decoder is scored against the token it has just been given and learns to copy it; needs the engine; free-running generation (TrainEngine.generate) is meaningful only for a model trained this way; DESIGN.md section 5i
FREE_RUNNING_EVAL = False           # False | True: the test stage also measures FREE-RUNNING reconstruction -- encode, generate from the start token on the key/value-cache decoder, compare with the input on the device (exact match, token edit distance, positional matches; TrainEngine.reconstruct): fr_exact / fr_token_acc / fr_edit_rate in the stage line and log, free_running_* columns in decoded_sentences.*, reconstruction_by_factor.md; needs DECODER_NEXT_TOKEN, the engine and a single process; the best-checkpoint decision does not change; KVQ_FREE_RUNNING_EVAL; DESIGN.md section 5l
FREE_RUNNING_EVAL_VAL = False       # with FREE_RUNNING_EVAL: every validation stage measures it as well (one generation per validation batch and epoch)
FREE_RUNNING_EVAL_BEAMS = 1         # int in 1 .. 8: 1 = greedy generation, more = the best hypothesis of a beam search of that width
PARAM_GROUPS = None                 # None (off) | list of {"match": pattern | [patterns], "lr_scale": float >= 0 (1), "weight_decay": float >= 0 (WEIGHT_DECAY)}: fnmatch patterns over the engine's parameter names (engine.param_names()), first match wins, the rest trains under LR and WEIGHT_DECAY; e.g. [{"match": ["*.b", "*.ln.w", "*.ln2.w", "head.bias"], "weight_decay": 0.0}] (= kvq.engine.NO_DECAY); KVQ_PARAM_GROUPS (JSON); DESIGN.md section 5h
DECOUPLED_WEIGHT_DECAY = False      # False | True: torch.optim.AdamW's decoupled decay instead of Adam's coupled L2 term, in the engine's Adam kernel; KVQ_DECOUPLED_WD (0 / 1)
LR_WARMUP_STEPS = 0                 # int >= 0: the rate climbs as t / LR_WARMUP_STEPS over the first optimiser steps (0: off); multiplies the MultiStepLR factor
LR_DECAY = None                     # None | "linear" | "cosine": decay from the end of the warm-up to LR_MIN_RATIO * LR at step LR_TOTAL_STEPS, where it stays
LR_TOTAL_STEPS = None               # int > LR_WARMUP_STEPS, with LR_DECAY
LR_MIN_RATIO = None                 # float in [0, 1], with LR_DECAY (None: 0)

RUNS_DIR = "./runs/Bagon"
EXPORT_CHECKPOINT = True
EXPORT_TRAIN_STATE = False           # write <run dir>/bagon_train_state_last.pth (kvq/train_state.py): model, the engine's full training state (or optimiser + scheduler), the trainer's bookkeeping and the generators -- what RESUME_FROM continues from, bit for bit on the engine path; DESIGN.md section 5e
TRAIN_STATE_EVERY_EPOCHS = 1         # int >= 1: the file is rewritten at the end of every this-many-th epoch and of the last one (a save is a device-to-host copy of the flat buffers: profiles/train_state.md has its cost beside an epoch's)
RESUME_FROM = None                   # None | a run directory or a training-state file: continue that run IN ITS directory at the epoch behind the stored one; N_EPOCHS is the new total, the batch-deciding constants and the engine's options must be the stored ones (refused otherwise)
WANDB_SILENT = "true"
WANDB_PROJECT_NAME = "kindergarten-vq-vae"
WANDB_GROUP = "Bagon"
WANDB_JOB_TYPE = "train"
WANDB_MODE = "disabled"
WANDB_WATCH_MODEL = False
WANDB_LOG_CODE = False

for _k in [k for k in list(globals()) if k.isupper()]:
    _v = _os.environ.get("KVQ_" + _k)
    if _v is not None:
        try:
            globals()[_k] = _ast.literal_eval(_v)
        except (ValueError, SyntaxError):
            globals()[_k] = _v
if isinstance(MAX_GRAD_NORM, str):       # KVQ_MAX_GRAD_NORM=inf is no python literal; empty = off (as TrainEngine reads the variable)
    MAX_GRAD_NORM = float(MAX_GRAD_NORM) if MAX_GRAD_NORM.strip() else None
_v = _os.environ.get("KVQ_GRAD_ACCUM", "").strip()      # the variable TrainEngine itself reads; it wins over KVQ_GRAD_ACCUM_STEPS; empty = unset
if _v:
    try:
        GRAD_ACCUM_STEPS = _ast.literal_eval(_v)
    except (ValueError, SyntaxError):
        GRAD_ACCUM_STEPS = _v
if isinstance(GRAD_ACCUM_STEPS, str) and not GRAD_ACCUM_STEPS.strip():
    GRAD_ACCUM_STEPS = 1
if isinstance(GRAD_ACCUM_STEPS, bool) or not isinstance(GRAD_ACCUM_STEPS, int) or GRAD_ACCUM_STEPS < 1:
    raise ValueError(f"GRAD_ACCUM_STEPS (KVQ_GRAD_ACCUM) must be an integer >= 1, got {GRAD_ACCUM_STEPS!r}")
_v = _os.environ.get("KVQ_WEIGHT_EMA", "").strip()      # the variable TrainEngine itself reads; it wins over KVQ_WEIGHT_EMA_DECAY; empty = unset
if _v:
    try:
        WEIGHT_EMA_DECAY = _ast.literal_eval(_v)
    except (ValueError, SyntaxError):
        WEIGHT_EMA_DECAY = _v
if isinstance(WEIGHT_EMA_DECAY, str) and not WEIGHT_EMA_DECAY.strip():
    WEIGHT_EMA_DECAY = None
if WEIGHT_EMA_DECAY is not None and (isinstance(WEIGHT_EMA_DECAY, bool) or not isinstance(WEIGHT_EMA_DECAY, (int, float))
                                     or not 0 < WEIGHT_EMA_DECAY < 1):
    raise ValueError(f"WEIGHT_EMA_DECAY (KVQ_WEIGHT_EMA) must be None or a float in (0, 1), got {WEIGHT_EMA_DECAY!r}")
if not isinstance(WEIGHT_EMA_EVAL, bool):
    raise ValueError(f"WEIGHT_EMA_EVAL (KVQ_WEIGHT_EMA_EVAL) must be True or False, got {WEIGHT_EMA_EVAL!r}")
if isinstance(LOSS_IGNORE_PAD, str) and not LOSS_IGNORE_PAD.strip():      # KVQ_LOSS_IGNORE_PAD= (empty) = unset, as TrainEngine reads the variable
    LOSS_IGNORE_PAD = False
if LOSS_IGNORE_PAD in (0, 1) and not isinstance(LOSS_IGNORE_PAD, bool) and _os.environ.get("KVQ_LOSS_IGNORE_PAD", "").strip() in ("0", "1"):
    LOSS_IGNORE_PAD = bool(LOSS_IGNORE_PAD)      # the environment spells the switch 0 / 1, as TrainEngine reads it
if not isinstance(LOSS_IGNORE_PAD, bool):
    raise ValueError(f"LOSS_IGNORE_PAD (KVQ_LOSS_IGNORE_PAD) must be True or False (0 or 1 in the environment), got {LOSS_IGNORE_PAD!r}")
if DECODER_NEXT_TOKEN in (0, 1) and not isinstance(DECODER_NEXT_TOKEN, bool) and _os.environ.get("KVQ_DECODER_NEXT_TOKEN", "").strip() in ("0", "1"):
    DECODER_NEXT_TOKEN = bool(DECODER_NEXT_TOKEN)      # the environment may spell the switch 0 / 1, as KVQ_LOSS_IGNORE_PAD
if not isinstance(DECODER_NEXT_TOKEN, bool):
    raise ValueError(f"DECODER_NEXT_TOKEN (KVQ_DECODER_NEXT_TOKEN) must be True or False (0 or 1 in the environment), got {DECODER_NEXT_TOKEN!r}")
for _k in ("FREE_RUNNING_EVAL", "FREE_RUNNING_EVAL_VAL"):      # the environment may spell the switches 0 / 1, as KVQ_DECODER_NEXT_TOKEN
    if globals()[_k] in (0, 1) and not isinstance(globals()[_k], bool) and _os.environ.get("KVQ_" + _k, "").strip() in ("0", "1"):
        globals()[_k] = bool(globals()[_k])
    if not isinstance(globals()[_k], bool):
        raise ValueError(f"{_k} (KVQ_{_k}) must be True or False (0 or 1 in the environment), got {globals()[_k]!r}")
if isinstance(FREE_RUNNING_EVAL_BEAMS, bool) or not isinstance(FREE_RUNNING_EVAL_BEAMS, int) or not 1 <= FREE_RUNNING_EVAL_BEAMS <= 8:
    raise ValueError(f"FREE_RUNNING_EVAL_BEAMS (KVQ_FREE_RUNNING_EVAL_BEAMS) must be an integer in 1 .. 8, got {FREE_RUNNING_EVAL_BEAMS!r}")
_v = _os.environ.get("KVQ_DECOUPLED_WD", "").strip()      # the variable TrainEngine itself reads; it wins over KVQ_DECOUPLED_WEIGHT_DECAY; empty = unset
if _v:
    DECOUPLED_WEIGHT_DECAY = {"0": False, "1": True}.get(_v, _v)
if isinstance(DECOUPLED_WEIGHT_DECAY, str) and not DECOUPLED_WEIGHT_DECAY.strip():
    DECOUPLED_WEIGHT_DECAY = False
if isinstance(PARAM_GROUPS, str):        # KVQ_PARAM_GROUPS is JSON, as TrainEngine reads it (a list of plain dicts is a python literal as well); empty = off
    import json as _json
    try:
        PARAM_GROUPS = _json.loads(PARAM_GROUPS) if PARAM_GROUPS.strip() else None
    except ValueError:
        raise ValueError(f"PARAM_GROUPS (KVQ_PARAM_GROUPS) must be a JSON list of groups, got {PARAM_GROUPS!r}") from None
for _k in ("LR_WARMUP_STEPS", "LR_DECAY", "LR_TOTAL_STEPS", "LR_MIN_RATIO"):      # KVQ_<NAME>= (empty) = unset, as TrainEngine reads the variables
    if isinstance(globals()[_k], str) and not globals()[_k].strip():
        globals()[_k] = 0 if _k == "LR_WARMUP_STEPS" else None
if (PARAM_GROUPS, DECOUPLED_WEIGHT_DECAY, LR_WARMUP_STEPS, LR_DECAY, LR_TOTAL_STEPS, LR_MIN_RATIO) != (None, False, 0, None, None, None):
    # one set of rules: the engine's own check_* methods (static, no device needed) judge the values; a refusal names the constant
    def _check_optimiser_options():
        from kvq._ffi import KvqError
        from kvq.engine import TrainEngine as E
        checked, what = {}, None
        try:
            for what, check in (("PARAM_GROUPS", E.check_param_groups), ("DECOUPLED_WEIGHT_DECAY", E.check_decoupled_weight_decay),
                                ("LR_WARMUP_STEPS", E.check_lr_warmup_steps), ("LR_DECAY", E.check_lr_decay),
                                ("LR_TOTAL_STEPS", E.check_lr_total_steps), ("LR_MIN_RATIO", E.check_lr_min_ratio)):
                checked[what] = check(globals()[what])
            what = "LR_TOTAL_STEPS / LR_MIN_RATIO"
            E.check_lr_schedule(checked["LR_WARMUP_STEPS"], checked["LR_DECAY"], checked["LR_TOTAL_STEPS"], checked["LR_MIN_RATIO"])
        except KvqError as e:
            raise ValueError(f"{what} (KVQ_{what.split(' ')[0]}): {e}") from None
        return checked["LR_DECAY"]
    LR_DECAY = _check_optimiser_options()        # ("none" means None)
    del _check_optimiser_options
if isinstance(TRAIN_STATE_EVERY_EPOCHS, bool) or not isinstance(TRAIN_STATE_EVERY_EPOCHS, int) or TRAIN_STATE_EVERY_EPOCHS < 1:
    raise ValueError(f"TRAIN_STATE_EVERY_EPOCHS (KVQ_TRAIN_STATE_EVERY_EPOCHS) must be an integer >= 1, got {TRAIN_STATE_EVERY_EPOCHS!r}")
if isinstance(RESUME_FROM, str) and not RESUME_FROM.strip():      # KVQ_RESUME_FROM= (empty) = unset
    RESUME_FROM = None
if RESUME_FROM is not None and not isinstance(RESUME_FROM, str):
    raise ValueError(f"RESUME_FROM (KVQ_RESUME_FROM) must be None or the path of a run directory / training-state file, got {RESUME_FROM!r}")
if not isinstance(EXPORT_TRAIN_STATE, bool):
    raise ValueError(f"EXPORT_TRAIN_STATE (KVQ_EXPORT_TRAIN_STATE) must be True or False, got {EXPORT_TRAIN_STATE!r}")


def get_config() -> dict:
    return {k.lower(): v for k, v in globals().items() if k.isupper() and not k.startswith("_")}
