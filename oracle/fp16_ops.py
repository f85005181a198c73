"""CPU ORACLE (test infrastructure, NOT product code) -- the stages of a tdnet_opts.precision = 1 ("fp16 MFMA") frame behind c4, each
restated from the stage BEFORE it with the operand rounding of the HIP kernels.

oracle/tdnet_ref.py rounds nothing, so a whole fp16-mode frame can only be held to it at 3e-2.  Here every function takes the handle's own
previous stage (tdnet_get_stage) and evaluates one stage from it on the operands as the kernels round them, so that what is left is the
kernel's accumulation and, for a stage of two convs, the few intermediate values that sit on a rounding boundary:

  * weights: BatchNorm folded in fp64 and stored as fp32 (td_weights.h fold), then -- for a conv on the fp16 MFMA -- rounded to fp16
    when packed (td_conv_h.h conv_pack_weights_h); biases stay fp32;
  * a conv runs on the fp16 MFMA when Cin % 64 == 0 (td_weights.h plan_conv's h16 rule: every conv behind c4): its input map is rounded to
    fp16, round to nearest even, when staged (or stored as fp16 by the kernel in front: the same rounding);
  * the attention (td_attn_h.h) rounds q AFTER the fp32 multiplication by log2(e) / 8, k and V' = fc(v) as they are, and the unnormalised
    P = 2^(s - row maximum); its row sum is that of the rounded P.  The kernels evaluate softmax(q k^T) (v W^T) + b where the reference
    evaluates (softmax(q k^T) v) W^T + b (td_frame.h launch_chain);
  * the pyramid, the LayerNorm statistics and expression, the classifier and the upsample are fp32 kernels: no rounding.

acc: torch.float64 (the reference proper) or torch.float32 (the same graph accumulated in fp32, as the MFMA does in some order): the
difference of the two is the checker's own measure of what accumulation order may cost.  rounded = False: the same graph with no rounding
at all -- what a test uses to prove that its gates tell the two apart.  Only tests/ may import this file."""
import numpy as np
import torch
import torch.nn.functional as F

from . import tdnet_ref as R

SCALE_LOG2E = np.float32(1.4426950408889634) / np.float32(8.0)        # td_launch.h run_attention: log2(e) / sqrt(d_k), in fp32


def half(t):
    """fp32 values held in any float tensor -> fp16 (round to nearest even) -> back."""
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


class Fp16Stages:
    def __init__(self, spec, state_dict, acc=torch.float64, rounded=True, round_p=False):
        self.name = spec.name
        self.acc, self.rounded, self.round_p = acc, rounded, round_p
        self.sd = {k: torch.as_tensor(np.asarray(v)).double() for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        self.psp_path_num, self.pids = R.REF_PSP[spec.name]
        self.atn_order = R.REF_ATN_ORDER[spec.name]

    # ---- operands -------------------------------------------------------------------------------------------------------------------
    def _r(self, t):
        return half(t) if self.rounded else t

    def fold(self, wkey, bkey, bn):
        """td_weights.h fold: (w * scale) and (bias * scale + shift) formed in fp64 and stored as fp32; then the fp16 packing."""
        w = self.sd[wkey]
        cb = self.sd[bkey] if bkey else torch.zeros(w.shape[0], dtype=torch.float64)
        scale, shift = torch.ones_like(cb), torch.zeros_like(cb)
        if bn:
            scale = self.sd[bn + ".weight"] / torch.sqrt(self.sd[bn + ".running_var"] + 1e-5)
            shift = self.sd[bn + ".bias"] - self.sd[bn + ".running_mean"] * scale
        w32 = (w * scale[:, None, None, None]).float().double()
        b32 = (cb * scale + shift).float().double()
        assert w.shape[1] % 64 == 0, "every conv behind c4 has Cin % 64 == 0: the fp16 MFMA (plan_conv's h16 rule)"
        return self._r(w32), b32

    def conv(self, x, w, b, stride=1, pad=0):
        """One fp16-MFMA conv: the input rounded when staged, exact products, accumulation in self.acc, the fp32 bias added."""
        return F.conv2d(self._r(x).to(self.acc), w.to(self.acc), None, stride, pad).double() + b[None, :, None, None]

    # ---- Encoding (transformer.py:28-56; td_frame.h encode_frame) from the handle's z [1, C, h, w] ---------------------------------------
    def z_from_c4(self, c4, pos):
        """fp32 kernels: the reference's pyramid slice in fp64."""
        return R.pyramid_pooling(torch.as_tensor(c4).double(), self.sd, "psp%d" % (pos + 1), self.psp_path_num, self.pids[pos]).numpy()

    def v_cur(self, z, pos, stride=1):
        w, b = self.fold("enc%d.w_vs.0.conv.weight" % (pos + 1), "enc%d.w_vs.0.conv.bias" % (pos + 1), "")
        return self.conv(torch.as_tensor(z).double(), w, b, stride).numpy()

    def qk(self, z, pos, branch, stride=1):
        """w_qs / w_ks: conv + BN + LeakyReLU -> conv.  Returns (result [n, 64, h', w'], the intermediate map y, |w2| [64, 64]): y is the map
        whose rounding to fp16 the second conv's staging performs."""
        pre = "enc%d.w_%s" % (pos + 1, branch)
        w0, b0 = self.fold(pre + ".0.conv.weight", pre + ".0.conv.bias", pre + ".0.bn")
        w1, b1 = self.fold(pre + ".1.conv.weight", pre + ".1.conv.bias", "")
        y = F.leaky_relu(self.conv(torch.as_tensor(z).double(), w0, b0, stride), 0.01)
        return self.conv(y, w1, b1).numpy(), y.numpy(), w1[:, :, 0, 0].abs().numpy()

    # ---- attention chain (td_frame.h launch_chain + finish_frame) ---------------------------------------------------------------------------
    def _fc(self, x, name):
        """V' = x W^T on the fp16 MFMA, no bias (it is added behind P V'); V' itself is then rounded when re-tiled (k_attn_vt_h)."""
        w = self._r(self.sd[name + ".fc.0.conv.weight"][:, :, 0, 0])
        return (self._r(x).to(self.acc) @ w.to(self.acc).T).double()

    def _attn(self, q, k, vp, bias, resid, round_p):
        """-> (out [Lq, DV], A = sum_j p_j |v'_j|)"""
        if self.rounded:
            qs = half((q.float() * torch.tensor(SCALE_LOG2E)).double())
            s2 = (qs.to(self.acc) @ half(k).to(self.acc).T).double()
        else:
            s2 = q @ k.T * (float(np.log2(np.e)) / 8.0)
        p = torch.exp2(s2 - s2.max(1, keepdim=True)[0])
        if round_p:
            p = half(p.float().double())
        v = self._r(vp.float().double())
        den = p.sum(1, keepdim=True)
        out = (p.to(self.acc) @ v.to(self.acc)).double() / den + bias + resid
        return out, (p @ v.abs()) / den

    def feat(self, pos, q_cur, v_cur, fifo, round_p=None):
        """feat [Lq, DV] and the final step's A from q_cur [Lq, 64], v_cur [Lq, DV] and the FIFO [(cache_q, cache_k, cache_v)] oldest first
        (the handle's own stages of the earlier frames).  round_p: P rounded in the steps BEFORE the final one (None: self.round_p)."""
        rp = self.round_p if round_p is None else round_p
        t = lambda a: torch.as_tensor(np.asarray(a)).double()
        names = self.atn_order[pos]
        bias = lambda n: self.sd[n + ".fc.0.conv.bias"]
        if self.name == "td4":
            (q0, k0, v0), (q1, k1, v1), (q2, k2, v2) = [tuple(t(a) for a in e) for e in fifo]
            a, _ = self._attn(q1, k0, self._fc(v0, names[0]), bias(names[0]), v1, rp)            # v2 + V[1]
            b, _ = self._attn(q2, k1, self._fc(a, names[1]), bias(names[1]), v2, rp)             # v3 + V[2]
            out, amp = self._attn(t(q_cur), k2, self._fc(b, names[2]), bias(names[2]), t(v_cur), False)
        else:
            (q0, k0, v0), = [tuple(t(a) for a in e) for e in fifo]
            out, amp = self._attn(t(q_cur), k0, self._fc(v0, names[0]), bias(names[0]), t(v_cur), False)
        return out.numpy(), amp.numpy()

    # ---- head (td4_psp18.py:287-312; td_frame.h finish_frame) from the handle's feat [1, DV, h, w] -------------------------------------
    def ln(self, feat, pos):
        """fp32 kernels: the plane LayerNorm in fp64."""
        return R.layer_norm_hw(torch.as_tensor(feat).double(), self.sd, "layer_norm%d" % (pos + 1)).numpy()

    def lowres(self, feat, pos):
        """LayerNorm -> rounded to fp16 (k_ln_apply_h, or the head conv's staging) -> conv3x3 + BN + ReLU on the fp16 MFMA -> the fp32
        classifier.  Returns (low [1, NC, h, w], the LayerNorm map y, amp): one flipped rounding of y (2^-10 |y|) moves a hidden channel c by
        at most that times max|w2[c]| and a logit by at most that times amp = max_n sum_c |cls[n, c]| max|w2[c]|."""
        pre = "head%d.conv5" % (pos + 1)
        w2, b2 = self.fold(pre + ".0.weight", "", pre + ".1")
        y = torch.as_tensor(self.ln(feat, pos))
        hid = F.relu(self.conv(y, w2, b2, 1, 1))
        cls = self.sd[pre + ".4.weight"]
        low = F.conv2d(hid, cls, self.sd[pre + ".4.bias"])
        amp = float((cls[:, :, 0, 0].abs() @ w2.abs().amax((1, 2, 3))).max())
        return low.numpy(), y.numpy(), amp
