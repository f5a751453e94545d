"""Mean attention maps of the decoder -- counterpart of analyses/cross_attention/extract_model_cross_attention.py.

    PYTHONPATH=kindergarten-vq-vae_amd python3 kindergarten-vq-vae_amd/analyses/cross_attention/extract_model_cross_attention.py

Same wiring as the reference: dataset -> DataLoader(BATCH_SIZE) -> tokenizer(padding="max_length",
max_length=TOKENIZED_SENTENCE_MAX_LENGTH) (:64-68) -> encoder -> bottleneck -> decoder with the encoder's ids and mask (:73-83), and
the same result files in RESULTS_DIR:
    cross_attentions_mean_across_batch_size.pth   float32 [decoder layers, heads, S, S]   (:103, :107)
    attentions_mean_across_batch_size.pth         float32 [decoder layers, heads, S, S]   (:104, :108)
and, only with PER_SLOT_MEAN=True,
    cross_attentions_mean_across_num_batches.pth  float32 [decoder layers, batch size, heads, S, S]   (:94, :98)
    attentions_mean_across_num_batches.pth                                                           (:95, :99)
What differs:
  * where the work happens: the reference asks HuggingFace for output_attentions=True, copies every batch's
    [layers, B, heads, S, S] stack to the host and averages there -- "had to limit to 69 batches in order to avoid memory crashes"
    (:59-60).  Here the probabilities come from the engine's own kernels (TrainEngine.attention_maps -> kvq_attn_probs) and are
    summed per batch into device-resident f64 tables (kvq.census.AttentionCensus), read back once: no batch limit.
  * the reference saves `cross_attns` under BOTH names (:98-99, :107-108), so its attentions_* files hold the cross-attention
    maps; here each tensor is saved under its own name.
  * the batch-size mean is the mean over all sentences; the reference's mean over batches of the mean over a batch's slots is the
    same number when every batch is full, and weighs the sentences of a short last batch more otherwise.  The per-slot mean
    drops a short last batch (the reference's torch.stack would fail on one).
  * the model is the Shelgon of models/shelgon3 (the reference's script builds the non-runnable `models.shelgon` v1) or, with
    MODEL_NAME="Bagon", the plain autoencoder.
Constants can be overridden from the environment as KVQ_<NAME>=<python literal>, as in models/shelgon3/config.py.
"""
import ast
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))      # package root (common/, kvq/, models/, dsentences/)

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from common.consts import *  # noqa: E402,F401,F403
from dsentences.dataset import dSentencesDataset  # noqa: E402
from dsentences.synthetic import write_corpus  # noqa: E402
from kvq.census import AttentionCensus  # noqa: E402
from kvq.tokenizer import load_tokenizer  # noqa: E402
from models.bagon.Bagon import Bagon  # noqa: E402
from models.shelgon3.Shelgon import Shelgon  # noqa: E402
from models.shelgon3.VectorQuantizer import VectorQuantizer  # noqa: E402

MODEL_NAME = "Shelgon"                                                                       # :23
SENTENCES_PATH = "./data/dSentences/dSentences_sentences.npy"                                # run_conf["dataset_path"] (:32)
SYNTHETIC_SENTENCES = 65536          # written when the corpus is absent (it is git-ignored upstream)
BATCH_SIZE = 2048                                                                            # :34
TOKENIZED_SENTENCE_MAX_LENGTH = 12                                                           # run_conf (:66)
TOKENIZER_ADD_SPECIAL_TOKENS = False                                                         # run_conf (:67)
TOKENIZER_NAME = "bert-base-uncased"
ENCODER_MODEL_NAME = "bert-base-uncased"
DECODER_MODEL_NAME = "bert-base-uncased"
COMPUTE_DTYPE = "bfloat16"
VQ_N_E = 9
VQ_E_DIM = 768
VQ_BETA = 0.1
CKPT_PATH = None                     # "./runs/Shelgon/<RUN_ID>/Shelgon_ckpt_loss_recon_val_best.pth" (:51); None = fresh weights
RUN_ID = "no_checkpoint"                                                                     # :25
RESULTS_DIR = None                   # default: ./runs/<MODEL_NAME>/<RUN_ID> (:27)
PER_SLOT_MEAN = False                # also write the *_mean_across_num_batches.pth pair: a [L, B, nh, S, S] accumulator per family
LIM_BATCHES = None                   # None = every batch (:60 stops at 69)

for _k in [k for k in list(globals()) if k.isupper()]:
    _v = os.environ.get("KVQ_" + _k)
    if _v is not None:
        try:
            globals()[_k] = ast.literal_eval(_v)
        except (ValueError, SyntaxError):
            globals()[_k] = _v


def maps_of_batches(model, tokenizer, batches, device, seq_len, add_special_tokens=False, per_slot_mean=False):
    """batches: iterables of lists of sentences.  -> (AttentionCensus, per-slot means {family: f32 [L, B, nh, S, S]} or None)"""
    cfg = model.decoder.config
    census = AttentionCensus(cfg.num_hidden_layers, cfg.num_attention_heads, seq_len, seq_len, device=device)
    slot_sum, n_full, batch_size = None, 0, None
    for sentences in batches:
        tokenized = tokenizer(list(sentences), return_tensors="pt", padding="max_length", max_length=seq_len,
                              add_special_tokens=add_special_tokens)                                                  # :64-68
        input_ids = tokenized.input_ids.to(device, non_blocking=True)
        attention_mask = tokenized.attention_mask.to(device, non_blocking=True)
        batch_size = batch_size or input_ids.shape[0]
        want_slots = per_slot_mean and input_ids.shape[0] == batch_size
        stacks = model.attention_maps(input_ids, attention_mask, census=census, per_sentence=want_slots)             # :73-86
        if want_slots:
            if slot_sum is None:
                slot_sum = {f: torch.zeros_like(t, dtype=torch.float64) for f, t in stacks.items()}
            for f, t in stacks.items():
                slot_sum[f] += t
            n_full += 1
    slots = {f: (t / n_full).to(torch.float32).cpu() for f, t in slot_sum.items()} if slot_sum is not None else None   # :94-95
    return census, slots


def write_results(means: dict, slots, results_dir: str) -> None:
    os.makedirs(results_dir, exist_ok=True)
    names = {"cross": "cross_attentions", "dec_self": "attentions"}
    if slots is not None:
        for f, name in names.items():                                                                                 # :98-99
            torch.save(slots[f], f"{results_dir}/{name}_mean_across_num_batches.pth")
    for f, name in names.items():                                                                                     # :107-108
        torch.save(means[f], f"{results_dir}/{name}_mean_across_batch_size.pth")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("the analysis needs an MI355X: the attention-map kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if not os.path.exists(SENTENCES_PATH):
        write_corpus(os.path.dirname(SENTENCES_PATH), SYNTHETIC_SENTENCES, seed=DS_GEN_SEED, suffix="")
    ds = dSentencesDataset(SENTENCES_PATH)                                                                            # :32
    dl = DataLoader(ds, batch_size=BATCH_SIZE, num_workers=0)                                                         # :36-39
    torch.manual_seed(0)
    dtype = getattr(torch, COMPUTE_DTYPE)
    if MODEL_NAME == "Shelgon":                                                                                       # :43-48
        vq = VectorQuantizer(n_e=VQ_N_E, e_dim=VQ_E_DIM, beta=VQ_BETA, vq_codebook_init_values=None)
        vq.materialize_min_encodings = False
        model = Shelgon(encoder_model_name=ENCODER_MODEL_NAME, vector_quantizer=vq, decoder_model_name=DECODER_MODEL_NAME,
                        compute_dtype=dtype).to(device)
    elif MODEL_NAME == "Bagon":
        model = Bagon(encoder_model_name=ENCODER_MODEL_NAME, decoder_model_name=DECODER_MODEL_NAME, compute_dtype=dtype).to(device)
    else:
        raise ValueError(f"{MODEL_NAME} NOT supported. Supported models: Shelgon, Bagon")
    if CKPT_PATH:
        model.load_state_dict(torch.load(CKPT_PATH, map_location=device)["model_state_dict"])                         # :51
    model.eval()                                                                                                      # :50
    torch.set_grad_enabled(False)                                                                                     # :52
    tokenizer = load_tokenizer(TOKENIZER_NAME)                                                                        # :54

    def batches():
        for b, batch in enumerate(dl):
            if LIM_BATCHES is not None and b >= LIM_BATCHES:
                break
            yield batch["sentence"]
    census, slots = maps_of_batches(model, tokenizer, batches(), device, TOKENIZED_SENTENCE_MAX_LENGTH, TOKENIZER_ADD_SPECIAL_TOKENS,
                                    PER_SLOT_MEAN)
    means = census.results()
    results_dir = RESULTS_DIR or f"./runs/{MODEL_NAME}/{RUN_ID}"
    write_results(means, slots, results_dir)
    print(f"{census.count} sentences, maps {tuple(means['cross'].shape)} -> {results_dir}")
    return means


if __name__ == "__main__":
    main()
