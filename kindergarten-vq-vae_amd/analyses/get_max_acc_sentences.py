"""The perfectly reconstructed sentences of a run -- counterpart of analyses/get_max_acc_sentences.py.

    PYTHONPATH=kindergarten-vq-vae_amd python3 kindergarten-vq-vae_amd/analyses/get_max_acc_sentences.py

Reads <RUN_DIR>/decoded_sentences.feather (what models/bagon/main.py and models/shelgon3/main.py write; the .csv they write when
feather is unavailable is read when the .feather is absent), keeps the rows with sentence_acc > 0.999, sorts them by
input_sentence, renumbers them (the old index stays as the column "index", as reset_index() leaves it) and writes
    <RUN_DIR>/decoded_sentences_max_acc_only.md
    <RUN_DIR>/decoded_sentences_max_acc_only.feather      (.csv when feather is unavailable)
-- the table analyses/latent_arithmetics/ and analyses/latent_traversals/ start from.  Host work only.
sentence_acc is the per-sentence accuracy the run's step reported: with LOSS_IGNORE_PAD / KVQ_LOSS_IGNORE_PAD=1 (DESIGN.md section
5g) that is the accuracy over the sentence's real tokens, so the filter then keeps the sentences whose WORDS were all reconstructed;
nothing changes here.
FREE_RUNNING = True (KVQ_FREE_RUNNING) filters on free_running_exact instead: the sentences the latent ALONE gave back when the
decoder generated from a start token (a run made with FREE_RUNNING_EVAL) -- teacher-forced accuracy hands the
decoder the true prefix at every position and is not the number that matters for such a model (section 5i).  A table of a run made
without the option has no such column: an error that names it.
Constants can be overridden from the environment as KVQ_<NAME>=<python literal>, as in models/shelgon3/config.py.
"""
import ast
import os

MODEL_NAME = "Bagon"
RUN_ID = "no_checkpoint"
RUN_DIR = None                       # default: ./runs/<MODEL_NAME>/<RUN_ID>
DECODED_SENTENCES_DF_PATH = None     # default: <RUN_DIR>/decoded_sentences.feather
MAX_ACC_THRESHOLD = 0.999
FREE_RUNNING = False                 # False: sentence_acc > MAX_ACC_THRESHOLD | True: free_running_exact (KVQ_FREE_RUNNING)

for _k in [k for k in list(globals()) if k.isupper()]:
    _v = os.environ.get("KVQ_" + _k)
    if _v is not None:
        try:
            globals()[_k] = ast.literal_eval(_v)
        except (ValueError, SyntaxError):
            globals()[_k] = _v


def read_table(path: str):
    """The DataFrame at `path` (.feather or .csv); a missing .feather falls back to the .csv beside it."""
    import pandas as pd
    base, ext = os.path.splitext(path)
    if ext == ".feather" and os.path.exists(path):
        try:
            return pd.read_feather(path)
        except ImportError as e:          # feather needs pyarrow
            print(f"[analyses] feather import unavailable ({e}); trying {base}.csv")
    csv = path if ext == ".csv" else base + ".csv"
    if not os.path.exists(csv):
        raise FileNotFoundError(f"neither {path} nor {csv} exists")
    return pd.read_csv(csv)


def write_table(df, path: str) -> str:
    """df to `path` (.feather), or to the .csv beside it when feather is unavailable; returns the file written."""
    base, ext = os.path.splitext(path)
    if ext == ".feather":
        try:
            df.to_feather(path)
            return path
        except ImportError as e:
            print(f"[analyses] feather export unavailable ({e}); writing CSV instead")
    df.to_csv(base + ".csv", index=False)
    return base + ".csv"


def max_acc_only(decoded_sentences, threshold: float = 0.999, free_running: bool = False):
    """Rows with sentence_acc > threshold -- free_running: rows whose free_running_exact is true --, sorted by input_sentence
    (ascending), index reset."""
    if free_running:
        if "free_running_exact" not in decoded_sentences.columns:
            raise KeyError("FREE_RUNNING: the table has no column 'free_running_exact' -- the run was made without FREE_RUNNING_EVAL "
                           "(models/*/config.py), or none of its decoded stages evaluated free-running")
        # (a .csv stores the flags as text; rows of stages that did not evaluate are missing values: not kept)
        flag = decoded_sentences["free_running_exact"].map(lambda v: v is True or str(v).strip().lower() in ("true", "1", "1.0"))
        kept = decoded_sentences[flag]
    else:
        kept = decoded_sentences[decoded_sentences["sentence_acc"] > threshold]
    kept = kept.sort_values(by="input_sentence", ascending=True)
    return kept.reset_index()


def main():
    run_dir = RUN_DIR or f"./runs/{MODEL_NAME}/{RUN_ID}"
    src = DECODED_SENTENCES_DF_PATH or f"{run_dir}/decoded_sentences.feather"
    if not isinstance(FREE_RUNNING, bool):
        raise ValueError(f"FREE_RUNNING (KVQ_FREE_RUNNING) must be True or False, got {FREE_RUNNING!r}")
    kept = max_acc_only(read_table(src), MAX_ACC_THRESHOLD, FREE_RUNNING)
    out = os.path.splitext(src)[0] + "_max_acc_only"
    try:
        kept.to_markdown(out + ".md", index=False)
    except ImportError as e:              # to_markdown needs tabulate
        print(f"[analyses] markdown export unavailable ({e}); writing a plain-text table instead")
        with open(out + ".md", "w") as f:
            f.write(kept.to_string(index=False))
    written = write_table(kept, out + ".feather")
    print(f"{len(kept)} sentences with " + ("free_running_exact" if FREE_RUNNING else f"sentence_acc > {MAX_ACC_THRESHOLD}") + f" -> {written}")
    return kept


if __name__ == "__main__":
    main()
