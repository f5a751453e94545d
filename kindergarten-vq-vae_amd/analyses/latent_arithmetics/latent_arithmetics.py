"""Latent arithmetic on a generative factor -- counterpart of analyses/latent_arithmetics/latent_arithmetics_Bagon.py.

    PYTHONPATH=kindergarten-vq-vae_amd python3 kindergarten-vq-vae_amd/analyses/latent_arithmetics/latent_arithmetics.py

Same experiment as the reference (:24-139): from the perfectly reconstructed sentences take those whose GENERATIVE_FACTOR is
FACTOR_VALUE_NEG ("past") and FACTOR_VALUE_AFF ("present"), form v = enc(neg) - enc(aff), feed enc(neg sentences) + v to the decoder
as encoder_hidden_states with the sentences' own decoder ids, and compare the arg-max reconstructions with the originals.
What differs:
  * where the work happens: encoder, decoder and LM head run on the engine's kernels (model.encode_latents / decode_latents); the
    two groups are summed per batch into device-resident f64 tables (kvq.census.LatentCensus) and the shift is one kernel
    (kvq_latent_shift), so nothing is kept per sentence and N_SENTENCES = None takes every sentence (the reference stops at 300);
  * v is the difference of the two group MEANS per position; the reference subtracts the i-th "present" sentence from the i-th
    "past" one, which needs equally many of each and pairs unrelated sentences;
  * MODEL_NAME = "Shelgon" is served too: the shifted encoder output goes through the quantiser first (quantize=True);
  * the reference prints; here the sentences are written to <RESULTS_DIR>/latent_arithmetics.feather (.csv when feather is
    unavailable): input_sentence, recon_sentence (the unshifted latent decoded), edited_sentence.
Without <RUN_DIR>/decoded_sentences_max_acc_only.* the table is built from the dSentences corpus and its factor labels (written
synthetically when absent), as the other analyses do.
Constants can be overridden from the environment as KVQ_<NAME>=<python literal>, as in models/shelgon3/config.py.
With KVQ_LOSS_IGNORE_PAD=1 the engine behind model.decode_latents scores real tokens only: acc / acc_per_sentence
of decode() are then real-token accuracies and recon_ids carries the pad id at pads; nothing changes here.
"""
import ast
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))      # package root (common/, kvq/, models/, dsentences/, analyses/)

import torch  # noqa: E402

from analyses.get_max_acc_sentences import read_table, write_table  # noqa: E402
from common.consts import *  # noqa: E402,F401,F403
from dsentences.synthetic import write_corpus  # noqa: E402
from kvq.census import LatentCensus  # noqa: E402
from kvq.tokenizer import load_tokenizer  # noqa: E402
from models.bagon.Bagon import Bagon  # noqa: E402
from models.bagon.Trainer import explicit_latent_classes_labels  # noqa: E402
from models.shelgon3.Shelgon import Shelgon  # noqa: E402
from models.shelgon3.VectorQuantizer import VectorQuantizer  # noqa: E402

MODEL_NAME = "Bagon"                                                                         # :15
RUN_ID = "no_checkpoint"                                                                     # :17
RUN_DIR = None                       # default: ./runs/<MODEL_NAME>/<RUN_ID> (:19)
DECODED_SENTENCES_DF_PATH = None     # default: <RUN_DIR>/decoded_sentences_max_acc_only.feather (:21)
GENERATIVE_FACTOR = "verb_tense"                                                             # :25
FACTOR_VALUE_NEG = "past"                                                                    # :28
FACTOR_VALUE_AFF = "present"                                                                 # :32
N_SENTENCES = None                   # per group; None = all of them (:35 stops at 300)
ALPHA = 1.0                          # enc + ALPHA * v
SENTENCES_PATH = "./data/dSentences/dSentences_sentences.npy"
LATENT_CLASSES_LABELS_PATH = "./data/dSentences/dSentences_latent_classes_labels.npy"
SYNTHETIC_SENTENCES = 65536          # written when the corpus is absent (it is git-ignored upstream)
BATCH_SIZE = 2048
TOKENIZED_SENTENCE_MAX_LENGTH = 12                                                           # run_conf (:69)
TOKENIZER_ADD_SPECIAL_TOKENS = False                                                         # run_conf (:67)
TOKENIZER_NAME = "bert-base-uncased"
ENCODER_MODEL_NAME = "bert-base-uncased"
DECODER_MODEL_NAME = "bert-base-uncased"
COMPUTE_DTYPE = "bfloat16"
VQ_N_E = 9
VQ_E_DIM = 768
VQ_BETA = 0.1
CKPT_PATH = None                     # "<RUN_DIR>/bagon_ckpt_loss_recon_val_best.pth" (:55); None = fresh weights
RESULTS_DIR = None                   # default: <RUN_DIR>
FREE_RUNNING = False                 # True (or --free-running on the command line): the plain and the edited latent are GENERATED from each sentence's first token (model.generate_from_latents) instead of decoded against the sentence's own ids; for a model trained with DECODER_NEXT_TOKEN
NUM_BEAMS = 1                        # N > 1 (or --num-beams N on the command line; with free running): the plain and the edited sentence are the best of N hypotheses of beam search (model.generate_from_latents(num_beams=N)); the table gains recon_ / edited_ score, runner_up_<i> and runner_up_<i>_score columns
SAMPLES = 0                          # N > 0 (or --samples N; free-running generation, one beam): every latent is generated N more times, sampled with seeds SEED .. SEED + N - 1 (model.generate_from_latents(temperature, top_k, top_p, seed, want_scores=True)); the table gains sample_<i> / sample_<i>_score (and edited_sample_<i> / edited_sample_<i>_score) columns
TEMPERATURE = 1.0                    # --temperature T: of the samples
TOP_K = 0                            # --top-k K: the samples draw from the K most probable tokens (0 = off)
TOP_P = 1.0                          # --top-p P: ... from the shortest prefix of them whose mass reaches P (1 = off)
SEED = 0                             # --seed S: the first sample's seed

for _k in [k for k in list(globals()) if k.isupper()]:
    _v = os.environ.get("KVQ_" + _k)
    if _v is not None:
        try:
            globals()[_k] = ast.literal_eval(_v)
        except (ValueError, SyntaxError):
            globals()[_k] = _v


def corpus_table(sentences_path, labels_path, n_synthetic):
    """input_sentence + the named generative factors of every corpus sentence: the columns of decoded_sentences_max_acc_only."""
    import numpy as np
    import pandas as pd
    if not (os.path.exists(sentences_path) and os.path.exists(labels_path)):
        write_corpus(os.path.dirname(sentences_path), n_synthetic, seed=DS_GEN_SEED, suffix="")
    sentences, labels = np.load(sentences_path).tolist(), torch.as_tensor(np.load(labels_path))
    rows = [dict(input_sentence=s, **explicit_latent_classes_labels(l)) for s, l in zip(sentences, labels)]
    return pd.DataFrame(rows).sort_values(by="input_sentence", ascending=True).reset_index(drop=True)


def _batches(sentences, batch_size):
    for i in range(0, len(sentences), batch_size):
        yield sentences[i:i + batch_size]


def _tokenize(tokenizer, sentences, device, seq_len, add_special_tokens):
    t = tokenizer(list(sentences), return_tensors="pt", padding="max_length", max_length=seq_len, add_special_tokens=add_special_tokens)
    return t.input_ids.to(device, non_blocking=True), t.attention_mask.to(device, non_blocking=True)


def beam_columns(tokenizer, beam_ids, beam_scores, prefix=""):
    """score of the best hypothesis and the runner-ups of one sentence as table columns: beam_ids [W, L], beam_scores [W], best first"""
    texts, scores = tokenizer.batch_decode(beam_ids.cpu()), beam_scores.cpu().tolist()
    cols = {prefix + "score": scores[0]}
    for i in range(1, len(texts)):
        cols[f"{prefix}runner_up_{i}"] = texts[i]
        cols[f"{prefix}runner_up_{i}_score"] = scores[i]
    return cols


def num_beams_switch(default):
    """--num-beams N on the command line, else the configured constant"""
    argv = sys.argv[1:]
    return int(argv[argv.index("--num-beams") + 1]) if "--num-beams" in argv else int(default)


def sampling_switch(samples, temperature, top_k, top_p, seed, num_beams=1):
    """--samples N --temperature T --top-k K --top-p P --seed S on the command line, else the configured constants:
    dict(samples, temperature, top_k, top_p, seed).  Samples are drawn, not searched: refused together with num_beams > 1.
    A sample is always generated free-running (there is nothing to draw in a teacher-forced decode)."""
    argv = sys.argv[1:]
    opt = lambda flag, default, kind: kind(argv[argv.index(flag) + 1]) if flag in argv else kind(default)
    s = dict(samples=opt("--samples", samples, int), temperature=opt("--temperature", temperature, float), top_k=opt("--top-k", top_k, int),
             top_p=opt("--top-p", top_p, float), seed=opt("--seed", seed, int))
    if s["samples"] < 0:
        raise SystemExit(f"--samples must be >= 0, got {s['samples']}")
    if s["samples"] and num_beams > 1:
        raise SystemExit(f"--samples {s['samples']} together with --num-beams {num_beams}: samples are drawn with one beam (sampled beams are not supported)")
    return s


def sample_columns(tokenizer, i, ids, score, prefix=""):
    """one sample of one sentence as table columns, as beam_columns adds the runner-ups"""
    return {f"{prefix}sample_{i}": tokenizer.batch_decode(ids.unsqueeze(0).cpu())[0], f"{prefix}sample_{i}_score": float(score)}


def latent_arithmetics(model, tokenizer, s_neg, s_aff, s_edit, device, seq_len, batch_size, add_special_tokens=False, alpha=1.0,
                       free_running=False, num_beams=1, sampling=None):
    """-> (LatentCensus over group 0 = s_aff, group 1 = s_neg; rows of original / reconstructed / edited sentences of s_edit)"""
    H = model.encoder.config.hidden_size
    quantize = hasattr(model, "vector_quantizer")
    census = LatentCensus(2, seq_len, H, device=device)
    for group, sentences in ((0, s_aff), (1, s_neg)):                                        # :60-90
        for batch in _batches(sentences, batch_size):
            ids, mask = _tokenize(tokenizer, batch, device, seq_len, add_special_tokens)
            census.add(model.encode_latents(ids, mask, quantize=False)["z"], group)
    rows = []
    for batch in _batches(s_edit, batch_size):                                               # :94-139
        ids, mask = _tokenize(tokenizer, batch, device, seq_len, add_special_tokens)
        z = model.encode_latents(ids, mask, quantize=False)["z"]
        if free_running:                        # what the latent says by itself: the decoder sees the first token and its own output
            start = ids[:, :1].contiguous()
            plain_out = model.generate_from_latents(z, seq_len, start, quantize=quantize, num_beams=num_beams)
            edited_out = model.generate_from_latents(census.shift(z, 1, 0, alpha=alpha), seq_len, start, quantize=quantize, num_beams=num_beams)
            plain, edited = plain_out["ids"], edited_out["ids"]
        else:
            plain = model.decode_latents(z, ids, mask, quantize=quantize)["recon_ids"]
            edited = model.decode_latents(census.shift(z, 1, 0, alpha=alpha), ids, mask, quantize=quantize)["recon_ids"]
        first = len(rows)
        for s, r, e in zip(batch, tokenizer.batch_decode(plain.cpu()), tokenizer.batch_decode(edited.cpu())):
            rows.append({"input_sentence": s, "recon_sentence": r, "edited_sentence": e})
            if free_running and num_beams > 1:  # the runner-up hypotheses and the sums of log-probabilities
                i = len(rows) - 1 - first
                rows[-1].update(beam_columns(tokenizer, plain_out["beam_ids"][i], plain_out["beam_scores"][i], "recon_"))
                rows[-1].update(beam_columns(tokenizer, edited_out["beam_ids"][i], edited_out["beam_scores"][i], "edited_"))
        if sampling and sampling["samples"]:    # the same captured step every time: the seed lives in the state
            start = ids[:, :1].contiguous()
            for prefix, lat in (("", z), ("edited_", census.shift(z, 1, 0, alpha=alpha))):
                for n in range(sampling["samples"]):
                    out = model.generate_from_latents(lat, seq_len, start, quantize=quantize, temperature=sampling["temperature"],
                                                      top_k=sampling["top_k"], top_p=sampling["top_p"], seed=sampling["seed"] + n, want_scores=True)
                    for i in range(len(batch)):
                        rows[first + i].update(sample_columns(tokenizer, n, out["ids"][i], out["scores"][i], prefix))
    return census, rows


def main():
    import pandas as pd
    free_running, num_beams = bool(FREE_RUNNING) or "--free-running" in sys.argv[1:], num_beams_switch(NUM_BEAMS)
    sampling = sampling_switch(SAMPLES, TEMPERATURE, TOP_K, TOP_P, SEED, num_beams)
    if not torch.cuda.is_available():
        raise SystemExit("the analysis needs an MI355X: the encoder, decoder and latent kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    run_dir = RUN_DIR or f"./runs/{MODEL_NAME}/{RUN_ID}"
    src = DECODED_SENTENCES_DF_PATH or f"{run_dir}/decoded_sentences_max_acc_only.feather"
    try:
        sentences_df = read_table(src)                                                       # :23
    except FileNotFoundError:
        sentences_df = corpus_table(SENTENCES_PATH, LATENT_CLASSES_LABELS_PATH, SYNTHETIC_SENTENCES)
    all_neg = sentences_df[sentences_df[GENERATIVE_FACTOR] == FACTOR_VALUE_NEG]["input_sentence"].tolist()     # :27-33
    all_aff = sentences_df[sentences_df[GENERATIVE_FACTOR] == FACTOR_VALUE_AFF]["input_sentence"].tolist()
    if not all_neg or not all_aff:
        raise SystemExit(f"no sentence with {GENERATIVE_FACTOR} == {FACTOR_VALUE_NEG!r} / {FACTOR_VALUE_AFF!r} in the table")
    n = N_SENTENCES or max(len(all_neg), len(all_aff))
    s_neg, s_aff, s_edit = all_neg[:n], all_aff[:n], all_neg[-n:]                            # :37-38, :94 (head, head, tail)
    torch.manual_seed(0)
    dtype = getattr(torch, COMPUTE_DTYPE)
    if MODEL_NAME == "Bagon":                                                                # :49-55
        model = Bagon(encoder_model_name=ENCODER_MODEL_NAME, decoder_model_name=DECODER_MODEL_NAME, compute_dtype=dtype).to(device)
    elif MODEL_NAME == "Shelgon":
        vq = VectorQuantizer(n_e=VQ_N_E, e_dim=VQ_E_DIM, beta=VQ_BETA, vq_codebook_init_values=None)
        vq.materialize_min_encodings = False
        model = Shelgon(encoder_model_name=ENCODER_MODEL_NAME, vector_quantizer=vq, decoder_model_name=DECODER_MODEL_NAME,
                        compute_dtype=dtype).to(device)
    else:
        raise ValueError(f"{MODEL_NAME} NOT supported. Supported models: Bagon, Shelgon")
    if CKPT_PATH:
        model.load_state_dict(torch.load(CKPT_PATH, map_location=device)["model_state_dict"])
    model.eval()
    torch.set_grad_enabled(False)                                                            # :45
    tokenizer = load_tokenizer(TOKENIZER_NAME)
    census, rows = latent_arithmetics(model, tokenizer, s_neg, s_aff, s_edit, device, TOKENIZED_SENTENCE_MAX_LENGTH, BATCH_SIZE,
                                      TOKENIZER_ADD_SPECIAL_TOKENS, ALPHA, free_running=free_running, num_beams=num_beams, sampling=sampling)
    results_dir = RESULTS_DIR or run_dir
    os.makedirs(results_dir, exist_ok=True)
    written = write_table(pd.DataFrame(rows), f"{results_dir}/latent_arithmetics.feather")
    counts = census.results()["count"].tolist()
    changed = sum(r["recon_sentence"] != r["edited_sentence"] for r in rows)
    print(f"{counts[1]} {FACTOR_VALUE_NEG} / {counts[0]} {FACTOR_VALUE_AFF} sentences, {len(rows)} edited ({changed} changed) -> {written}")
    return rows


if __name__ == "__main__":
    main()
