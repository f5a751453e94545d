"""f64 reference of the reconstruction loss over the counted rows only (the kvq_*_ignore entry points of csrc/kvq_ce.hip,
DESIGN.md section 5g): tests/_pointwise_ref.py's ce_ref extended by an ignore set.  Runs on the CPU;
tests/test_loss_ignore_host.py holds it against F.cross_entropy(ignore_index=...) and its autograd gradient."""
import torch

import _pointwise_ref as R


def ce_ignore_ref(x, target, ignore_index, g_loss=1.0):
    """From the up-cast logits x [N, V] (CPU) and target [N]: a row is IGNORED iff target == ignore_index (which may lie outside
    [0, V)), every other row is counted.  Returns ce_ref's dict with
      counted [N] bool ; count (int) ; c = g_loss / max(count, 1)
      lse, row_loss : ce_ref's on counted rows, 0 on ignored ones ; pred : first arg-max, ignore_index on ignored rows
      grad, cp      : c (softmax - onehot) and c softmax on counted rows, 0 on ignored ones
      loss = sum(row_loss) / count, acc = hits / count over the counted rows -- both 0 when count == 0 (torch: NaN)
      absmax        : ce_ref's on counted rows, 0 on ignored ones (whatever an ignored row holds, NaN included, is never looked at)."""
    x = x.detach().cpu().double()
    t = target.detach().cpu().long()
    counted = t != int(ignore_index)
    count = int(counted.sum())
    c = float(g_loss) / max(count, 1)
    xs = torch.where(counted[:, None], x, torch.zeros_like(x))              # ignored rows: their contents are selected away
    ts = torch.where(counted, t, torch.zeros_like(t))
    ref = R.ce_ref(xs, ts, c)
    z = torch.zeros_like(ref["lse"])
    out = dict(counted=counted, count=count, c=c,
               lse=torch.where(counted, ref["lse"], z), row_loss=torch.where(counted, ref["row_loss"], z),
               pred=torch.where(counted, ref["pred"], torch.full_like(ref["pred"], int(ignore_index))),
               grad=torch.where(counted[:, None], ref["grad"], torch.zeros_like(ref["grad"])),
               cp=torch.where(counted[:, None], ref["cp"], torch.zeros_like(ref["cp"])),
               absmax=torch.where(counted, ref["absmax"], z))
    hits = int(((out["pred"] == t) & counted).sum())
    out["hits"] = hits
    out["loss"] = float(out["row_loss"].sum()) / count if count else 0.0
    out["acc"] = hits / count if count else 0.0
    return out


def seq_acc_ignore_ref(pred, target, ignore_index):
    """[B] f32: hits over each sentence's counted tokens / their number, the integer ratio formed in f64 and rounded to f32;
    0 for a sentence without a counted token.  pred / target [B, S] int64."""
    pred, target = pred.detach().cpu().long(), target.detach().cpu().long()
    counted = target != int(ignore_index)
    hits = ((pred == target) & counted).sum(1).double()
    cnt = counted.sum(1).double()
    return torch.where(cnt > 0, hits / cnt.clamp(min=1), torch.zeros_like(cnt)).float()
