"""QVidModel: frame encoder + VQ + flow-guided frame decoder behind the reference's dict API.

Host-side mirror of the inference half of the reference's
`models/skip_vid_generator/models/quantized_video_model.py` (`forward` mode dispatch :45-98,
`preprocess_input` :101-122, `encode` :773-819, `decode` :822-918, `vid_step_decode` :920-949):
same constructor, same modes, same dict keys in and out, `ValueError` on an unknown mode.

Differences that do not change results:
  * the context ring of skip features is a circular buffer (slot permutation instead of the
    reference's overlapping in-place shift, :898-900/:946, which torch >= 1.8 rejects anyway);
  * re-encoding a synthesized frame inside the decode loop (:875-878) skips the vector
    quantiser, whose output that loop discards;
  * `embed_code` + two transposes (:832-833) is one gather kernel writing NCHW.
`eval_img_to_img_generator` (:460-480), the frame autoencoder's validation L1, runs; `eval_reconstruction` adds the quantiser's loss
and codebook usage from the same pass.  Training modes, layout decoders and continuous codes are outside the hot path and raise.
"""
import torch

from .skip_autoencoder import SkipGANDecoder, SkipGANEncoder, prepare_packed_modules
from ..modules.quantize import VectorQuantizer
from ccvs_amd import ops
from ccvs_amd.tools.utils import to_cuda
from ccvs_amd.models import load_network, print_network

_TRAIN_MODES = ("img_to_img_generator", "vid_to_vid_generator", "img_discriminator", "img_discriminator_reg", "vid_discriminator_reg",
                "vid_discriminator")


class QVidModel(torch.nn.Module):
    def __init__(self, opt, is_train=False, is_main=True, logger=None):
        super().__init__()
        if is_train:
            raise NotImplementedError("training is outside the MI355X hot path")
        self.opt = opt
        self.is_main = is_main
        self.initialize_networks(is_train)
        self.logger = logger if self.is_main else None

    def forward(self, data, fake_data={}, mode='', log=False, suffix="", cond_frames=None, global_iter=None, motion=False):
        if mode in _TRAIN_MODES:
            raise NotImplementedError(f"mode '{mode}' (training) is outside the MI355X hot path")
        if mode not in ("eval_img_to_img_generator", "img_encoder", "vid_encoder", "img_decoder", "vid_decoder", "vid_step_decoder"):
            raise ValueError(f"mode '{mode}' is invalid")
        real_img, real_vid, code, state_code, inter, interl, cond_inter = self.preprocess_input(data)
        if mode == 'eval_img_to_img_generator':
            return self.eval_reconstruction(real_img, log, global_iter)["l1"]
        if mode == 'img_encoder':
            return self.encode(real_img, None, "img", log, suffix, global_iter)
        if mode == 'vid_encoder':
            return self.encode(real_vid, None, "vid", log, suffix, global_iter)
        if mode == 'img_decoder':
            return self.decode(code, state_code, inter, interl, cond_inter, "img", log, suffix, None, global_iter)
        if mode == 'vid_decoder':
            return self.decode(code, state_code, inter, interl, cond_inter, "vid", log, suffix, cond_frames, global_iter, motion=motion)
        return self.vid_step_decode(code, inter, cond_inter)

    def preprocess_input(self, data, is_fake=False):
        """quantized_video_model.py:101-122: the caller's dict is updated with device tensors."""
        for key in ("z", "img", "layout", "vid", "code", "state_code", "inter", "interl", "cond_inter"):
            data[key] = to_cuda(data, key)
        if 0 not in getattr(data["layout"], "shape", (0,)):
            raise NotImplementedError("layout conditioning is outside the MI355X hot path")
        return data["img"], data["vid"], data["code"], data["state_code"], data["inter"], data["interl"], data["cond_inter"]

    def initialize_networks(self, is_train):
        """quantized_video_model.py:125-205 (inference nets only)."""
        opt = self.opt
        if getattr(opt, "use_layout", False) or getattr(opt, "is_continuous", False):
            raise NotImplementedError("layout / continuous-code variants are outside the MI355X hot path")
        self.net_e = None
        if opt.use_enc:
            if opt.enc_model != "skipgan":
                raise ValueError
            self.net_e = SkipGANEncoder(opt).cuda()
        self.net_q = VectorQuantizer(opt.z_num, opt.z_size, beta=0.25, mult=getattr(opt, "z_mult", 1),
                                     normalize=getattr(opt, "normalize_out", False)).cuda()
        self.net_g = None
        if opt.use_dec:
            if opt.dec_model != "skipgan":
                raise ValueError
            self.net_g = SkipGANDecoder(opt).cuda()
        if self.is_main:
            load_ema = getattr(opt, "use_ema", False)
            bd = getattr(opt, "block_delta", None)
            sfx = "_ema" if load_ema else ""
            self.net_g = load_network(self.net_g, "qvid_g" + sfx, opt, block_delta=bd)
            self.net_e = load_network(self.net_e, "qvid_e" + sfx, opt)
            self.net_q = load_network(self.net_q, "qvid_q" + sfx, opt, required=load_ema)

    @torch.no_grad()
    def prepare_packed(self):
        """Build, on the current stream, every kernel-ready weight form the networks cache lazily on first use (packed
        convolution weights of the chosen precision, fused heads, split Subpixel weights, the quantiser's transposed codebook).
        A caller that is about to use the model from SEVERAL streams (`Generator.run_pipelined`: the decode of batch i on decode
        stream i % D) calls this once and orders those streams behind it: the caches are plain Python attributes, nothing else
        orders a pack kernel on one stream before a reader on another.  Cheap when everything is already packed."""
        prepare_packed_modules(self)

    # ------------------------------------------------------------------ validation
    @torch.no_grad()
    def eval_reconstruction(self, img, log=False, global_iter=None):
        """quantized_video_model.py:460-480 (`compute_eval_img_to_img_generator_loss`) with the quantiser's diagnostics from the same
        pass: img [N, 3, H, W] -> encoder -> quantiser -> decoder on the frame's own skip features (the decoder's default
        arguments).  One encode and one decode per call.  Returns device tensors, nothing synchronised:
          "l1"          0-dim fp32, mean |img - fake_img|: what mode 'eval_img_to_img_generator' returns
          "quant_loss"  0-dim fp32, (1 + beta) mean((z_q - z)^2) (quantize.py:60-61)
          "perplexity"  0-dim fp32, exp of the entropy of the code frequencies (quantize.py:67-68)
          "codes_used"  0-dim int64, codes chosen at least once;  "code_counts" int32 [z_num]
          "code"        int64 [N, h * w];  "fake_img" [N, 3, H, W]
        With a logger and `log` the two images are logged under the reference's names (:476-478)."""
        real_img = img if img.is_cuda else img.cuda()
        z, inter_enc = self.net_e(real_img)
        z_q, q_loss, (perplexity, counts, idx) = self.net_q.forward_with_stats(z)
        fake_img, _ = self.net_g(z_q, [inter_enc])
        loss = ops.l1_mean(real_img, fake_img)
        if self.logger and log:
            self.logger.log_img("qvid_generator/eval_fake_img", fake_img[:16].float().cpu(), 4, global_iter, normalize=True, span=(-1, 1))
            self.logger.log_img("qvid_generator/eval_real_img", real_img[:16].float().cpu(), 4, global_iter, normalize=True, span=(-1, 1))
        return {"l1": loss, "quant_loss": q_loss, "perplexity": perplexity, "codes_used": (counts > 0).sum(), "code_counts": counts,
                "code": idx.view(z.shape[0], -1), "fake_img": fake_img}

    # ------------------------------------------------------------------ encode
    @torch.no_grad()
    def encode(self, data, layout, dtype, log, suffix, global_iter, quantize=True):
        """quantized_video_model.py:773-819 (discrete codes)."""
        z, inter_enc = self.net_e(data)
        empty = torch.tensor([])
        if not quantize:
            return {"code": empty, "state_code": empty, "inter": inter_enc, "interl": empty, "z": z}
        zq, _, info = self.net_q(z)
        code = info[2].view(z.shape[0], -1)
        return {"code": code, "state_code": empty, "inter": inter_enc, "interl": empty, "z": zq}

    # ------------------------------------------------------------------ decode
    def _embed(self, code, frames):
        """codes [B, frames*h*w] -> z [B, frames, C, h, w] (quantized_video_model.py:832-833)."""
        h, w = self.opt.z_shape[:2]
        z = self.net_q.embed_code_nchw(code, code.size(0) * frames, h, w)
        return z.view(code.size(0), frames, self.opt.z_size, h, w)

    @torch.no_grad()
    def decode(self, code, state_code, inter, interl, cond_inter, dtype, log, suffix, cond_frames, global_iter, motion=False):
        """quantized_video_model.py:822-918 (skip_mode 'enc' or 'dec', no layout).  motion: (ccvs_amd) where the clip goes through the
        frame loop, also return the decoder's motion (`decode_frames`): "motion", "warp", "flow_dt" beside the clip."""
        opt = self.opt
        h, w = opt.z_shape[:2]
        if dtype == "img":
            z = self.net_q.embed_code_nchw(code, code.size(0), h, w)
            fake, _ = self.net_g(z, [inter])
            return {dtype: fake, "layout": None}
        frames = code.size(1) // (h * w)
        if not (opt.use_inter and opt.dec_model == "skipgan" and inter[0].size(1) < opt.vid_len):
            fake, _ = self.net_g(self._embed(code, frames), [inter])
            return {dtype: fake, "layout": None}
        gen = self.decode_frames(lambda lo, hi: code[:, lo * h * w:hi * h * w], inter, cond_inter, motion=motion)
        while True:
            try:
                next(gen)
            except StopIteration as fin:
                if motion:
                    return {dtype: fin.value[0], "layout": None, **fin.value[1]}
                return {dtype: fin.value, "layout": None}

    def decode_stream(self, data, code_of, frames=None, motion=False):
        """`forward(mode='vid_decoder')` for a clip whose tokens arrive frame by frame (the token loop is still running): a generator
        that yields, before each piece of work, how many frames of tokens that piece needs (`decode_frames`) and returns the decoder's
        dict.  `data` as for the decoder, without "code"; `code_of(lo, hi)` -> the tokens [B, (hi - lo) * h * w] of frames lo .. hi - 1.
        Without the flow-guided frame loop (no `--q_use_inter`, or every frame given) the clip is ONE decoder call, as in `decode`
        (quantized_video_model.py:849-853): one piece that needs all `frames` frames of tokens."""
        opt = self.opt
        _, _, _, _, inter, _, cond_inter = self.preprocess_input(data)
        if not (opt.use_inter and opt.dec_model == "skipgan" and inter[0].size(1) < opt.vid_len):
            frames = int(frames if frames is not None else opt.vid_len)
            yield frames
            fake, _ = self.net_g(self._embed(code_of(0, frames), frames), [inter])
            return {"vid": fake, "layout": None}
        vid = yield from self.decode_frames(code_of, inter, cond_inter, motion=motion)
        if motion:
            return {"vid": vid[0], "layout": None, **vid[1]}
        return {"vid": vid, "layout": None}

    def decode_frames(self, code_of, inter, cond_inter, motion=False):
        """The frame loop of the flow-guided decode (quantized_video_model.py:855-918) as a generator: before the conditioning
        frames and before every new frame it yields the number of leading frames whose tokens it is about to read through
        `code_of(lo, hi)`, so a caller can run it beside the token loop that produces them (`Generator.run_pipelined`) -- or
        simply exhaust it (`decode`).  Every frame is embedded and decoded by the same launches either way.  Returns the clip.

        motion (ccvs_amd): also keep what the decoder estimated for every new frame -- the last level's flow
        towards the frame's first context and the mask its blend used, written by one launch per frame (`ops.flow_export`, reading
        the decoder's own rows in place) into "motion" [B, T, 3, H, W] -- and return (clip, {"motion", "warp", "flow_dt"}):
        "flow_dt"[t] = how many frames back that context lies (0: a frame without flow -- a conditioning frame, a frame decoded
        without context, a frame whose first context is not one of the clip's own frames; its motion is 0), "warp"[:, t] = frame
        t - dt of the clip back-warped by the flow alone (`SkipGANDecoder.backwarp_img`; frame t itself where there is no flow).
        The clip's launches and bits are the same with and without it."""
        opt = self.opt
        ctx = inter[0].size(1)
        batch = inter[0].size(0)
        fakes = []
        mot, flow_dt = None, [0] * ctx
        if ctx > 0:
            yield ctx
            fakes.append(self.net_g(self._embed(code_of(0, ctx), ctx), [inter])[0])   # conditioning frames, own skip features
        # context ring: `skip_memory` slots per level, newest last (quantized_video_model.py:864-866)
        mem = opt.skip_memory
        ring = []
        for feat in inter:
            r = feat.new_zeros(batch, mem, *feat.shape[2:])
            keep = min(ctx, mem)
            if keep:
                r[:, mem - keep:] = feat[:, ctx - keep:]
            ring.append(r)
        # The ring is circular: `order[p]` is the physical slot of logical position p (oldest .. newest), so
        # the per-frame "shift left by one" (quantized_video_model.py:895-901) moves no data, and contexts
        # are slot VIEWS (the reference's `feat[:, [-dt]]` list-index makes a copy per context and level).
        order = list(range(mem))
        curr = ctx
        has_cond = isinstance(cond_inter, list) and len(cond_inter) > 0
        if has_cond:
            ctx += 1
        n_new = opt.vid_len - ctx
        total = curr + n_new   # frames of the clip
        for step in range(n_new):
            yield curr + 1
            z = self._embed(code_of(curr, curr + 1), 1)
            inters = [[feat[:, order[mem - dt]: order[mem - dt] + 1] for feat in ring] for dt in opt.skip_context if dt <= curr]
            if has_cond:
                inters.append(cond_inter)
            lv_flows = lv_occs = None
            if opt.skip_mode == "enc":
                if motion:   # the same launches; the per-level features come back as views (nothing is cloned)
                    fake_img, _, lv_flows, lv_occs, _ = self.net_g(z, inters, return_all=True, inter_pre_warping=False, has_ctx=curr > 0)
                else:
                    fake_img, _ = self.net_g(z, inters, has_ctx=curr > 0)
                if motion:
                    mot, dt0 = self._export_motion(mot, curr, total, fake_img, lv_flows, lv_occs, len(inters))
                    flow_dt.append(dt0)
                if step == n_new - 1:
                    # the ring is local to this call and no frame follows: the reference's re-encode of the last
                    # synthesized frame (quantized_video_model.py:890-891) feeds slots nobody reads -- not run
                    fakes.append(fake_img)
                    break
                new_inter = self.encode(fake_img, None, "vid", False, None, None, quantize=False)["inter"]
            elif opt.skip_mode == "dec":
                fake_img, _, lv_flows, lv_occs, inter_dec = self.net_g(z, inters, return_all=True, inter_pre_warping=False, has_ctx=curr > 0)
                new_inter = list(reversed(inter_dec))
                if motion:
                    mot, dt0 = self._export_motion(mot, curr, total, fake_img, lv_flows, lv_occs, len(inters))
                    flow_dt.append(dt0)
            else:
                raise ValueError
            drop = opt.n_first if (getattr(opt, "keep_first", False) and curr >= mem) else 0   # logical slot that leaves
            order = order[:drop] + order[drop + 1:] + [order[drop]]
            for i in range(len(ring)):
                ring[i][:, order[-1]: order[-1] + 1] = new_inter[i]
            fakes.append(fake_img)
            curr += 1
        vid = torch.cat(fakes, dim=1)
        if not motion:
            return vid
        if mot is None:   # no new frame at all
            mot = vid.new_zeros(batch, vid.size(1), 3, *vid.shape[-2:], dtype=torch.float32)
        warp = vid.float().clone()
        for t, dt in enumerate(flow_dt):
            if dt > 0:
                ops.backwarp(vid[:, t - dt].float(), mot[:, t, :2], 1.0, out=warp[:, t])   # SkipGANDecoder.backwarp_img, written in place
        return vid, {"motion": mot, "warp": warp, "flow_dt": flow_dt}

    def _export_motion(self, mot, t, total, fake_img, lv_flows, lv_occs, k):
        """One new frame's motion into slot t of the clip's buffer `mot` ([B, total, 3, H, W], made of zeros at the first call):
        returns (mot, the dt of the frame's first context or 0).  Nothing is written for a frame decoded without flow (no context:
        `net_g` then returns no level) or whose first context is not a frame of the clip (the conditioning end frame)."""
        opt = self.opt
        if mot is None:
            mot = fake_img.new_zeros(fake_img.size(0), total, 3, *fake_img.shape[-2:], dtype=torch.float32)
        dts = [dt for dt in opt.skip_context if dt <= t]
        if not (lv_flows and dts):
            return mot, 0
        flow, occ = lv_flows[-1], lv_occs[-1]
        n, _, h, w = flow.shape
        # `flow | occ` are channel slices of one tensor (InterBlock.forward_fused's `fo`): seen again as its three planes, in place
        if occ.data_ptr() == flow.data_ptr() + 8 * h * w and occ.stride(0) == flow.stride(0) and flow.stride()[1:] == (h * w, w, 1):
            fo = flow.as_strided((n, 3, h, w), flow.stride())
        else:
            fo = torch.cat([flow, occ], dim=1)
        ops.flow_export(fo, k, float(self.net_g.last_flow_mult), mot, t)
        return mot, dts[0]

    @torch.no_grad()
    def vid_step_decode(self, code, inter, cond_inter):
        """quantized_video_model.py:920-949: decode one frame, re-encode it, re-quantise it."""
        opt = self.opt
        assert opt.use_inter and opt.dec_model == "skipgan"
        z = self._embed(code, 1)
        ctx = inter[0].size(1)
        inters = [[feat[:, [-dt]] for feat in inter] for dt in opt.skip_context if dt <= ctx]
        if isinstance(cond_inter, list) and len(cond_inter) > 0:
            inters.append(cond_inter)
        fake, _ = self.net_g(z, inters)
        new_data = self.encode(fake, None, None, False, None, None)
        if ctx < opt.skip_memory:
            inter = [torch.cat([feat, new_feat], dim=1) for feat, new_feat in zip(inter, new_data["inter"])]
        else:
            inter = [torch.cat([feat[:, 1:], new_feat], dim=1) for feat, new_feat in zip(inter, new_data["inter"])]
        return {"vid": fake, "inter": inter, "code": new_data["code"]}
