"""segmentation task -- caller of the hot path (mirror of tasks/mm_tasks/segmentation.py).

Keeps the reference's task surface: ``@register_task("segmentation", dataclass=SegmentationConfig)`` (:100) on
``FairseqTask`` when fairseq is importable, the config dataclasses field for field (``OFAConfig``
tasks/ofa_task.py:24-87, ``SegmentationConfig`` segmentation.py:37-98, so `--bpe-dir`, `--selected-cols`,
`--prompt-prefix`, `--category-list`, ... of run_scripts/IFSeg/coco_unseen.sh parse), ``setup_task`` (:108-135:
dictionary = dict.txt + <mask> + <code_i> + <bin_i> + (nseg+1) <seg_i>), ``build_model`` (:166),
``train_step`` (:190-222), ``valid_step`` (:225-229) and the ``sample`` dict layout of
data/mm_data/segmentation_dataset.py:110-127.  Data loading (TSV / mmseg pipeline) is out of scope (SURVEY.md
section 2.1): ``load_dataset`` refuses; samples for the bundled harness are synthetic tensors of the right shapes
(SURVEY.md 8d), and ``train_sample`` turns decoded images and label maps into a batch of that layout through the
training transform of the pipeline (ifseg_amd/augment.py, csrc/trainload.hip).
"""
import contextlib
import os
from dataclasses import dataclass, field
from typing import Optional

import torch

from ...registry import HAVE_FAIRSEQ, DataclassBase, TaskBase, register_task

BOS, PAD, EOS = 0, 1, 2
# "what is the segmentation map of the image? object:" BPE ids
PROMPT_IDS = (99, 16, 5, 2835, 1258, 5456, 9, 5, 2274, 116, 7626, 35)


def _f(default, help=""):
    return field(default=default, metadata={"help": help})


@dataclass
class OFAConfig(DataclassBase):
    """tasks/ofa_task.py:24-87"""
    data: Optional[str] = _f(None, "comma separated path to data list; valid data are always in the last")
    selected_cols: Optional[str] = _f(None, "selected cols")
    train_selected_cols: Optional[str] = _f(None, "selected cols for train")
    eval_selected_cols: Optional[str] = _f(None, "selected cols for valid/eval")
    bpe: Optional[str] = _f("gpt2", "which bpe to use")
    bpe_dir: Optional[str] = _f(None, "bpe dir")
    max_source_positions: int = _f(1024, "max number of tokens in the source sequence")
    max_target_positions: int = _f(1024, "max number of tokens in the target sequence")
    max_src_length: int = _f(128, "the maximum src sequence length")
    max_tgt_length: int = _f(30, "the maximum target sequence length")
    code_dict_size: int = _f(8192, "code dict size")
    patch_image_size: int = _f(480, "patch image size")
    orig_patch_image_size: int = _f(256, "patch image size")
    num_bins: int = _f(1000, "number of quantization bins")
    imagenet_default_mean_and_std: bool = _f(False, "imagenet normalize")
    constraint_range: Optional[str] = _f(None, "constraint range")


@dataclass
class SegmentationConfig(OFAConfig):
    """tasks/mm_tasks/segmentation.py:37-98"""
    eval_acc: bool = _f(True, "evaluation with accuracy")
    eval_args: Optional[str] = _f("{}", "generation args as JSON string")
    eval_print_samples: bool = _f(False, "print sample generations during validation")
    uses_ema: Optional[bool] = _f(False, "whether to use ema")
    add_object: bool = _f(False, "add object to encoder")
    max_object_length: int = _f(30, "the maximum object sequence length")
    valid_batch_size: int = _f(1, "valid batch size per step")
    scst: bool = _f(False, "Self-critical sequence training")
    scst_args: str = _f("{}", "generation args for Self-critical sequence training, as JSON string")
    artificial_image_type: str = _f("random", "random | gt_seg | upsampling | none")
    prompt_prefix: str = _f("", 'could be "what is the segmentation map of the image? object:"')
    num_seg_tokens: int = _f(150, "number of seg tokens")
    category_list: str = _f("", "list of semantic category words (comma separated)")
    epoch_row_count: int = _f(-1, "if -1, disabled.")
    artificial_image_on_device: bool = _f(False, "draw the artificial image of every image-free update on the device "
                                                 "(ifseg_amd/artificial.py); the sample's own aux_input is then ignored")


class SizeDictionary:
    """Stand-in for the fairseq Dictionary where dict.txt is not available (the GPU box): sizes and the symbols the
    path asks for (dict.txt 50260 lines + 4 specials + <mask> + 8192 <code_i> + 1000 <bin_i> + (nseg+1) <seg_i>)."""

    def __init__(self, n_base, nseg):
        self.n_base, self.nseg = n_base, nseg

    def __len__(self):
        return self.n_base + self.nseg + 1

    def __contains__(self, sym):
        return sym == "<mask>" or sym.startswith(("<seg_", "<bin_", "<code_"))

    def pad(self):
        return PAD

    def bos(self):
        return BOS

    def eos(self):
        return EOS

    def index(self, sym):
        if sym.startswith("<seg_"):
            return self.n_base + int(sym[5:-1])
        raise KeyError(sym)


@register_task("segmentation", dataclass=SegmentationConfig)
class SegmentationTask(TaskBase):
    def __init__(self, cfg=None, src_dict=None, tgt_dict=None, num_seg_tokens=None, patch_image_size=None,
                 n_base_vocab=59457, arch="segofa_base", src_len=None, category_token_ids=None):
        """`cfg, src_dict, tgt_dict` as in the reference (segmentation.py:102-107); the keyword form
        (`num_seg_tokens=...`) builds the config of the bundled harness with a size-only dictionary."""
        if cfg is None:
            cfg = SegmentationConfig(num_seg_tokens=15 if num_seg_tokens is None else num_seg_tokens,
                                     patch_image_size=512 if patch_image_size is None else patch_image_size,
                                     orig_patch_image_size=512 if patch_image_size is None else patch_image_size)
        super().__init__(cfg)
        self.arch = arch
        nseg = cfg.num_seg_tokens
        if src_dict is None:
            src_dict = tgt_dict = SizeDictionary(n_base_vocab, nseg)
        self.src_dict, self.tgt_dict = src_dict, tgt_dict
        self.uses_ema = getattr(cfg, "uses_ema", False)
        self.num_seg_tokens = nseg
        self.category_list = cfg.category_list
        self.seg_id_offset = tgt_dict.index("<seg_0>")
        # token ids of every category name, for the criterion's lazy seg-token initialisation where no BPE encoder
        # exists (the reference encodes `category_list` with task.bpe: seg_criterion.py:373-388)
        self.category_token_ids = category_token_ids
        self.prompt_ids = PROMPT_IDS              # the prompt in front of the category names (`train_sample`)
        self.bpe = None
        # L = bos + 12 prompt ids + class-name ids + eos: 36 / 215 / 239 for 15 / 150 / 171 classes
        self.src_len = src_len or {15: 36, 150: 215, 171: 239}.get(nseg, 14 + 2 * nseg)

    @classmethod
    def setup_task(cls, cfg, **kwargs):
        """segmentation.py:108-135.  Needs fairseq's Dictionary + `<bpe-dir>/dict.txt`."""
        if not HAVE_FAIRSEQ:
            raise RuntimeError("SegmentationTask.setup_task loads dict.txt through fairseq's Dictionary; without fairseq "
                               "construct SegmentationTask(num_seg_tokens=...) directly")
        dicts = []
        for _ in range(2):
            d = cls.load_dictionary(os.path.join(cfg.bpe_dir, "dict.txt"))
            d.add_symbol("<mask>")
            for i in range(cfg.code_dict_size):
                d.add_symbol("<code_{}>".format(i))
            for i in range(cfg.num_bins):
                d.add_symbol("<bin_{}>".format(i))
            for i in range(cfg.num_seg_tokens + 1):
                d.add_symbol("<seg_{}>".format(i))
            dicts.append(d)
        return cls(cfg, dicts[0], dicts[1])

    @property
    def source_dictionary(self):
        return self.src_dict

    @property
    def target_dictionary(self):
        return self.tgt_dict

    def load_dataset(self, split, epoch=1, combine=False, **kwargs):
        raise NotImplementedError("ifseg_amd: the TSV / mmseg data pipeline (data/mm_data/segmentation_dataset.py) is out "
                                  "of scope -- import the reference's own `tasks` next to `ifseg_amd.models` "
                                  "(INTEGRATION.md section 1) or feed samples in the collater's layout")

    def build_model(self, cfg=None):
        """segmentation.py:166-174 / ofa_task.py:167-185 (the BPE encoder and the vestigial sequence generator of the
        reference's build_model are data / decode plumbing: `ifseg_amd.sequence_generator` is built on demand)."""
        from ...models.segofa.segofa import SegOFAModel, recipe_args
        if cfg is None or not hasattr(cfg, "encoder_normalize_before"):
            over = {k: getattr(cfg, k) for k in ("arch", "dropout", "encoder_drop_path_rate", "decoder_drop_path_rate")
                    if cfg is not None and getattr(cfg, k, None) is not None}
            cfg = recipe_args(over.pop("arch", self.arch), num_seg_tokens=self.cfg.num_seg_tokens,
                              patch_image_size=self.cfg.patch_image_size,
                              orig_patch_image_size=self.cfg.orig_patch_image_size, **over)
        model = SegOFAModel.build_model(cfg, self)
        self._build_bpe_from_dir()
        return model

    def _build_bpe_from_dir(self):
        """ofa_task.py:167-185: under fairseq the task owns the GPT-2 BPE encoder built from `--bpe-dir`
        (encoder.json / vocab.bpe); the criterion's lazy seg-token initialisation encodes the category names with it
        (seg_criterion.py:373-388).  Without fairseq, or when the files are absent, `category_token_ids` must be given
        (or `--init-seg-with-text=false`): `encode_category` says so."""
        if self.bpe is not None or not HAVE_FAIRSEQ:
            return
        bpe_dir = getattr(self.cfg, "bpe_dir", None)
        if not bpe_dir:
            return
        enc, voc = os.path.join(bpe_dir, "encoder.json"), os.path.join(bpe_dir, "vocab.bpe")
        if not (os.path.exists(enc) and os.path.exists(voc)):
            return
        from omegaconf import DictConfig
        self.bpe = self.build_bpe(DictConfig({"_name": "gpt2", "gpt2_encoder_json": enc, "gpt2_vocab_bpe": voc}))

    def build_generator(self, models, args=None, seq_gen_cls=None, extra_gen_cls_kwargs=None, prefix_allowed_tokens_fn=None):
        """tasks/ofa_task.py:187-260 with the task's eval_args ({"beam":5,"max_len":1024,"min_len":1024,...},
        coco_unseen.sh:111): the fixed-length decode of ifseg_amd/sequence_generator.py"""
        from ...sequence_generator import SequenceGenerator
        g = lambda k, d: getattr(args, k, d) if args is not None else d
        return SequenceGenerator(models, self.target_dictionary, beam_size=g("beam", 5), max_len=g("max_len", None),
                                 min_len=g("min_len", 1), temperature=g("temperature", 1.0))

    def build_segmenter(self, model, **kw):
        """images -> label maps at image resolution on this task's categories (ifseg_amd/predict.py); raw uint8 images of
        any size go through `Segmenter.segment_raw`, the evaluation transform of the data pipeline on the device; every keyword
        of the constructor passes through (`slide_views=True`: multi-scale + flip over sliding windows; `sieve=K`: regions
        below K pixels take their largest neighbour's label -- `evaluate_raw`, `calibrate_raw`, `render_raw` and
        `pseudo_label_raw` below hand it on with `sieve_connectivity` and `sieve_passes`)"""
        from ...predict import Segmenter
        return Segmenter(model, task=self, **kw)

    def evaluate_raw(self, model, images, label_maps, slide=None, **kw):
        """raw uint8 images and their label maps -> a `SegmentationScore` (aAcc / mIoU / mAcc through `.summary()`), counted on
        the device: `build_segmenter(model, ...).evaluate_raw(images, label_maps, ...)`.  Keywords of the Segmenter's constructor
        go to it, the others to `Segmenter.evaluate_raw`; `slide` (None, True or (crop, stride)) is its sliding-window switch,
        `confusion=True` asks for the class confusion matrix (`score.confusion`) beside the three histograms,
        `boundary_iou=True` (or a ratio of the diagonal) for Boundary IoU's band areas (`score.boundary`; "mBIoU" in the summary),
        `calibration=True` for how often a confidence is right (`score.calibration`; "ECE" in the summary,
        `score.precision_thresholds(target)` for `self_train_sample`'s thresholds),
        `trimap=True` (or a tuple of radii) for mIoU / accuracy within r pixels of a ground-truth contour (`score.trimap`;
        "trimap_mIoU" in the summary)."""
        ctor = ("category_token_ids", "prompt_ids", "upsample", "smooth_iters", "smooth_topk", "temperature", "crf_iters",
                "full_context_alignment", "label_dtype", "slide_views", "pamr_iters", "pamr_dilations", "sieve",
                "sieve_connectivity", "sieve_passes", "class_bias")
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in ctor if k in kw})
        return seg.evaluate_raw(images, label_maps, slide=slide, **kw)

    def calibrate_raw(self, model, images, label_maps, **kw):
        """raw uint8 images and their label maps -> a `TemperatureSweep`: one forward per batch scored at every temperature of
        `temperatures` (None: `predict.default_temperatures()`) on the device, `sweep.best()` being the temperature of lowest
        mean NLL: `build_segmenter(model, ...).calibrate_raw(images, label_maps, ...)`.  Keywords of the Segmenter's constructor
        go to it, the others to `Segmenter.calibrate_raw`."""
        ctor = ("category_token_ids", "prompt_ids", "upsample", "smooth_iters", "smooth_topk", "temperature", "crf_iters",
                "full_context_alignment", "label_dtype", "slide_views", "pamr_iters", "pamr_dilations", "sieve",
                "sieve_connectivity", "sieve_passes", "class_bias")
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in ctor if k in kw})
        return seg.calibrate_raw(images, label_maps, **kw)

    def bias_sweep_raw(self, model, images, label_maps, direction, **kw):
        """raw uint8 images and their label maps -> a `BiasSweep`: one forward per batch scored under every strength of
        `strengths` (None: `predict.default_bias_strengths()`) of the per-class bias `direction` on the device,
        `sweep.best()` being the strength of highest mIoU and `sweep.bias(...)` its vector for `class_bias`:
        `build_segmenter(model, ...).bias_sweep_raw(images, label_maps, direction, ...)`.  Keywords of the Segmenter's
        constructor (read from its signature; `class_bias` is the sweep's origin) go to it, the others to
        `Segmenter.bias_sweep_raw`."""
        import inspect
        from ...predict import Segmenter
        keywords = [k for k in inspect.signature(Segmenter.__init__).parameters if k not in ("self", "model", "task")]
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in keywords if k in kw})
        return seg.bias_sweep_raw(images, label_maps, direction, **kw)

    def render_raw(self, model, images, **kw):
        """raw uint8 images -> a list of `RenderResult(picture, labels, conf)`, the label maps coloured over the photos on the
        device: `build_segmenter(model, ...).render_raw(images, ...)`.  Keywords of the Segmenter's constructor go to it, the
        others to `Segmenter.render_raw`."""
        ctor = ("category_token_ids", "prompt_ids", "upsample", "smooth_iters", "smooth_topk", "temperature", "crf_iters",
                "full_context_alignment", "label_dtype", "slide_views", "pamr_iters", "pamr_dilations", "sieve",
                "sieve_connectivity", "sieve_passes", "class_bias")
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in ctor if k in kw})
        return seg.render_raw(images, **kw)

    def pseudo_label_raw(self, model, images, **kw):
        """unlabeled raw uint8 images -> a list of `PseudoLabelResult(labels, predicted, conf, kept)`, label maps that hold only
        the pixels the model is confident of: `build_segmenter(model, ...).pseudo_label_raw(images, ...)`.  Keywords of the
        Segmenter's constructor go to it, the others to `Segmenter.pseudo_label_raw` -- `min_region=K` and
        `region_connectivity` among them: connected regions of the filtered map below K pixels become 255 too, and the
        results carry `region_dropped`."""
        ctor = ("category_token_ids", "prompt_ids", "upsample", "smooth_iters", "smooth_topk", "temperature", "crf_iters",
                "full_context_alignment", "label_dtype", "slide_views", "pamr_iters", "pamr_dilations", "sieve",
                "sieve_connectivity", "sieve_passes", "class_bias")
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in ctor if k in kw})
        return seg.pseudo_label_raw(images, **kw)

    def regions_raw(self, model, images, **kw):
        """raw uint8 images -> a list of `RegionTable`, one row per connected region of each image's label map (class value,
        area, box, centroid sums, summed confidence) on the device: `build_segmenter(model, ...).regions_raw(images, ...)`.
        Keywords of the Segmenter's constructor (read from its signature) go to it, the others -- `min_region`,
        `connectivity`, `max_regions`, `ignore` and `segment_raw`'s -- to `Segmenter.regions_raw`."""
        import inspect
        from ...predict import Segmenter
        keywords = [k for k in inspect.signature(Segmenter.__init__).parameters if k not in ("self", "model", "task")]
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in keywords if k in kw})
        return seg.regions_raw(images, **kw)

    def export_raw(self, model, images, **kw):
        """raw uint8 images -> a list of `RunLengthMap`, each image's label map as its runs in COCO's run order on the device
        (`.to_coco(image_id, category_ids)` gives COCO stuff results): `build_segmenter(model, ...).export_raw(images, ...)`.
        Keywords of the Segmenter's constructor (read from its signature) go to it, the others -- `max_runs` and
        `segment_raw`'s -- to `Segmenter.export_raw`."""
        import inspect
        from ...predict import Segmenter
        keywords = [k for k in inspect.signature(Segmenter.__init__).parameters if k not in ("self", "model", "task")]
        seg = self.build_segmenter(model, **{k: kw.pop(k) for k in keywords if k in kw})
        return seg.export_raw(images, **kw)

    def self_train_sample(self, model, images, first_ordinal, trainer=None, confidence_weight=False, **kw):
        """One batch of self-training on unlabeled photographs: `pseudo_label_raw(model, images, **kw)` and then
        `train_sample(images, [r.labels ...], first_ordinal)` on the model's own confident pixels -> the batch
        `Trainer.train_step` takes; every pixel that was not kept carries the ignore class.  `raw_labels` (default: the
        train transform's) must agree with the transform's, else the classes would shift by one: ValueError.
        `trainer`: the Trainer of `model`.  With `Trainer(store_ema=True)` the labels come from its teacher -- the averaged
        weights, inside `trainer.ema_weights()` -- instead of the weights being trained (mean teacher; the remedy for the
        confirmation bias of labelling with the student).  Without `trainer`, or with one that keeps no teacher, `model` labels
        as it stands.  Not built: `ema_seed_model`, and a teacher for the fairseq plugin's own trainer (its `EMA` deep-copies
        the model, which is untested with the arena-backed parameters).
        confidence_weight: the labelling launch also writes every pixel's confidence as a loss weight
        (`pseudo_label_raw(return_weight=True)`), the transform carries the planes to the batch and the sample gains
        `"target_weight"` (uint8 [B, P*P]), which the criterion's weighted kernel reads: a kept pixel counts by how sure the
        teacher was of it instead of 0 or 1.
        `min_region=K`, `region_connectivity` (in `kw`, as every keyword of `pseudo_label_raw`): the labels and the weight
        planes leave without their connected regions below K pixels."""
        tf = getattr(self, "train_transform", None) or self.build_train_transform()
        if confidence_weight:
            kw["return_weight"] = True
        raw = kw.setdefault("raw_labels", tf.raw_labels)
        if bool(raw) != tf.raw_labels:
            raise ValueError("self_train_sample: raw_labels=%r, but the train transform was built with raw_labels=%r"
                             % (raw, tf.raw_labels))
        images = [images] if torch.is_tensor(images) else list(images)
        teacher = trainer is not None and getattr(trainer, "store_ema", False)
        if teacher and trainer.model is not model:
            raise ValueError("self_train_sample: `trainer` trains another model than the one given")
        with trainer.ema_weights() if teacher else contextlib.nullcontext():
            res = self.pseudo_label_raw(model, images, **kw)
        labels = [r.labels.to(tf.device) for r in res]
        if not confidence_weight:
            return self.train_sample(images, labels, first_ordinal)
        return self.train_sample(images, labels, first_ordinal, weights=[r.weight.to(tf.device) for r in res])

    def distill_sample(self, sample, model, teacher=None, trainer=None, full_context_alignment=False):
        """`sample` plus `"teacher_logits"`: what `SegCriterion(distill_weight=)` trains `model` on -> a new dict, the sample's own
        entries shared.  The teacher runs on `sample["net_input"]` in eval mode under `torch.no_grad()` and a CLONE of its padded
        per-patch logits (bf16 [B, P+1, npad]) is attached: the buffer itself is the engine's workspace, the next forward
        overwrites it.
        `teacher`: another SegOFAModel on the same device (Large for a Base student, say); its training flag is restored
        afterwards.  Another class count or feature grid than the student's: ValueError.
        `trainer` (and no `teacher`): the Trainer of `model`, built with `Trainer(store_ema=True)` -- the student's own averaged
        weights label the sample, inside `trainer.ema_weights()`, in eval mode (mean teacher with soft targets).  A trainer that
        keeps no teacher or trains another model: ValueError, as is giving neither.
        The sample is the static input of a captured step (`train_step(graph=True)`), so the tensor attached here is one too: a
        caller who captures must copy new teacher logits INTO that tensor (`sample["teacher_logits"].copy_(...)`) instead of
        attaching a fresh one.  A second model's engine shares the hardware queues with the student's, see README.
        Not built: a fairseq command-line flag, a teacher at another grid or class set, feature-level distillation."""
        if teacher is None and trainer is None:
            raise ValueError("distill_sample: give `teacher` (a second model) or `trainer` (Trainer(store_ema=True) of `model`)")
        if teacher is None:
            if not getattr(trainer, "store_ema", False):
                raise ValueError("distill_sample: `trainer` keeps no teacher (Trainer(store_ema=True)) and no `teacher` was given")
            if trainer.model is not model:
                raise ValueError("distill_sample: `trainer` trains another model than the one given")
        net = teacher if teacher is not None else model
        if teacher is not None:
            n_t, n_s = teacher.decoder.seg_embed_tokens.weight.shape[0], model.decoder.seg_embed_tokens.weight.shape[0]
            if n_t != n_s:
                raise ValueError("distill_sample: the teacher has %d classes, the student %d" % (n_t, n_s))
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad(), (trainer.ema_weights() if teacher is None else contextlib.nullcontext()):
                _, extra = net(**sample["net_input"], full_context_alignment=full_context_alignment)
                logits = extra["logits_padded"].clone()
                grid = tuple(extra["encoder_returns"]["image_embed_shape"][0])
        finally:
            net.train(was_training)
        if teacher is not None:
            h, w = sample["net_input"]["patch_images"].shape[-2:]
            # (the student's trunk has stride 16; at other image sizes the criterion's own shape check decides)
            if h % 16 == 0 and w % 16 == 0 and (h // 16, w // 16) != grid:
                raise ValueError("distill_sample: the teacher's feature grid is %s, the student's %s" % (grid, (h // 16, w // 16)))
        return dict(sample, teacher_logits=logits)

    def inference_step(self, generator, models, sample, prefix_tokens=None, constraints=None):
        """fairseq_task.py `inference_step` -> [B, max_len] seg-class indices of the best beam (segmentation.py:266-268)"""
        with torch.no_grad():
            return generator.generate(models, sample)

    def encode_category(self, text):
        """token ids of one category name (seg_criterion.py:375-385: BPE of ' <word>' per word, dictionary lookup)"""
        if self.bpe is not None:
            line = " ".join(self.bpe.encode(" {}".format(w.strip())) for w in text.strip().split())
            return self.tgt_dict.encode_line(line=line, add_if_not_exist=False, append_eos=False).long()
        raise RuntimeError("no BPE encoder on this task (fairseq + <bpe-dir>/encoder.json, vocab.bpe build one in "
                           "build_model): pass category_token_ids=[...] to SegmentationTask or --init-seg-with-text=false")

    def synthetic_sample(self, batch, device, seed=1234, image_hw=None):
        """Synthetic batch with the collater's layout (segmentation_dataset.py:41-129)."""
        nseg, S = self.cfg.num_seg_tokens, self.cfg.patch_image_size
        hw = image_hw or (S, S)
        g = torch.Generator().manual_seed(seed)
        L = self.src_len
        body = list(PROMPT_IDS)[: max(0, L - 2)]
        body += torch.randint(4, min(50000, self.seg_id_offset - 1), (max(0, L - 2 - len(body)),), generator=g).tolist()
        src = torch.tensor([BOS] + body + [EOS]).repeat(batch, 1)
        img = torch.randn(batch, 3, hw[0], hw[1], generator=g)
        tgt = torch.randint(0, nseg, (batch, hw[0] * hw[1]), generator=g) + self.seg_id_offset
        tgt = torch.cat([tgt, torch.full((batch, 1), EOS, dtype=torch.long)], 1)
        return {
            "id": list(range(batch)), "nsentences": batch, "ntokens": int(batch * (hw[0] * hw[1] + 1)),
            "net_input": {"src_tokens": src.to(device), "src_lengths": torch.full((batch,), L).to(device),
                          "patch_images": img.to(device), "patch_masks": torch.ones(batch, dtype=torch.bool, device=device),
                          "prev_output_tokens": torch.zeros(batch, 1, dtype=torch.long, device=device)},
            "target": tgt.to(device),
        }

    def synthetic_aux_sample(self, batch, device, seed=4321):
        """Image-free half of a batch in the collater's layout (segmentation_dataset.py:303-345, :85-107):
        a random low-res class map (``rand_k-1-33``) nearest-resized to the patch grid (EmbeddingBag ids of the
        class names; every "name" here is 1-3 random BPE ids) and to the image (targets).
        -> {"aux_input": {...}, "text2seg_target": [B, S*S+1]}"""
        import torch.nn.functional as F
        nseg, S = self.cfg.num_seg_tokens, self.cfg.patch_image_size
        hp = S // 16
        g = torch.Generator().manual_seed(seed)
        L = self.src_len
        name_len = torch.randint(1, 4, (nseg,), generator=g)
        names = [torch.randint(4, min(50000, self.seg_id_offset - 1), (int(k),), generator=g) for k in name_len]
        body = list(PROMPT_IDS)[: max(0, L - 2)]
        body += torch.randint(4, min(50000, self.seg_id_offset - 1), (max(0, L - 2 - len(body)),), generator=g).tolist()
        src = torch.tensor([BOS] + body + [EOS]).repeat(batch, 1)
        ids, ends, tgts = [], [], []
        for _ in range(batch):
            sh, sw = (int(v) for v in torch.randint(1, 33, (2,), generator=g))
            coarse = torch.randint(0, nseg, (1, 1, sh, sw), generator=g).float()
            low = F.interpolate(coarse, size=(hp, hp), mode="nearest").long().reshape(-1)
            high = F.interpolate(coarse, size=(S, S), mode="nearest").long().reshape(-1)
            ids.append(torch.cat([names[int(c)] for c in low]))
            ends.append(name_len[low].cumsum(0))
            tgts.append(torch.cat([high + self.seg_id_offset, torch.tensor([EOS])]))
        maxlen = max(t.numel() for t in ids)
        padded = torch.full((batch, maxlen), PAD, dtype=torch.long)
        for b, t in enumerate(ids):
            padded[b, : t.numel()] = t
        return {"aux_input": {"src_tokens": src.to(device), "src_lengths": torch.full((batch,), L).to(device),
                              "patch_images": padded.to(device), "patch_masks": torch.cat(ends).to(device),
                              "prev_output_tokens": torch.zeros(batch, 1, dtype=torch.long, device=device)},
                "text2seg_target": torch.stack(tgts).to(device)}

    def build_artificial_sampler(self, device, seed=1):
        """The generator of the image-free samples for `--artificial-image-type rand_k[-L-R]` (ifseg_amd/artificial.py) on
        this task's patch grid.  The class names come from where the criterion's lazy seg-token initialisation takes them:
        `category_token_ids`, else `category_list` through the BPE encoder; the 'unknown' name (id2rawtext's last entry,
        segmentation_dataset.py:183; never drawn) is `unknown_token_ids` / the BPE of " unknown", else an empty bag."""
        from ...artificial import ArtificialImageSampler, parse_artificial_image_type
        lr = parse_artificial_image_type(self.cfg.artificial_image_type)
        if lr is None:
            raise RuntimeError("artificial_image_type 'none': this task has no artificial image to draw")
        nseg = self.num_seg_tokens
        names = self.category_token_ids
        if names is None:
            cats = [x.strip() for x in self.category_list.split(",")] if self.category_list else []
            if not cats:
                raise RuntimeError("build_artificial_sampler: the task carries neither category_list (+ BPE) nor category_token_ids")
            names = [self.encode_category(" %s" % x) for x in cats]
        names = [torch.as_tensor(x, dtype=torch.long).reshape(-1) for x in names]
        if len(names) != nseg:
            raise AssertionError("%d category names for %d seg tokens" % (len(names), nseg))
        unknown = getattr(self, "unknown_token_ids", None)
        if unknown is None:
            unknown = self.encode_category(" unknown") if self.bpe is not None else torch.zeros(0, dtype=torch.long)
        hp = self.cfg.patch_image_size // 16
        return ArtificialImageSampler(names + [torch.as_tensor(unknown, dtype=torch.long)], self.seg_id_offset, hp, hp, lr[0], lr[1],
                                      seed=seed, device=device, bos=BOS, eos=EOS, pad=PAD)

    def build_train_transform(self, device="cpu", seed=1, **kw):
        """The training transform of the data pipeline for this task (ifseg_amd/augment.py: Resize(ratio_range), RandomCrop,
        RandomFlip, PhotoMetricDistortion, Normalize of segmentation_dataset.py:148-163 on raw uint8 images and raw label
        maps), with the task's patch size, class count and normalisation; on a GPU device it runs csrc/trainload.hip."""
        from ...augment import TrainTransform
        from ...imageio import HALF, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
        if getattr(self.cfg, "imagenet_default_mean_and_std", False):
            kw.setdefault("mean", IMAGENET_DEFAULT_MEAN)
            kw.setdefault("std", IMAGENET_DEFAULT_STD)
        else:
            kw.setdefault("mean", HALF)
            kw.setdefault("std", HALF)
        kw.setdefault("eos", EOS)
        self.train_transform = TrainTransform(self.cfg.patch_image_size, self.num_seg_tokens, self.seg_id_offset, seed=seed,
                                              device=device, **kw)
        return self.train_transform

    def _train_src_tokens(self):
        """bos + prompt + the category names + eos, as `predict.source_tokens` builds them for the Segmenter"""
        if getattr(self, "_train_src", None) is None:
            from ...predict import source_tokens
            names = self.category_token_ids
            if names is None:
                cats = [x.strip() for x in self.category_list.split(",")] if self.category_list else []
                if not cats:
                    raise RuntimeError("train_sample: the task carries neither category_list (+ BPE) nor category_token_ids")
                names = [self.encode_category(" %s" % x) for x in cats]
            self._train_src = source_tokens(names, self.prompt_ids, self.num_seg_tokens)
        return self._train_src

    def train_sample(self, images, labels, first_ordinal, weights=None):
        """Raw uint8 images [H0, W0, 3] (RGB) and raw uint8 label maps [H0, W0] of any sizes -> the batch `Trainer.train_step`
        takes, in `synthetic_sample`'s layout, through `build_train_transform`'s transform (built on first use, on the CPU,
        if the caller has not built one).  `first_ordinal` is the ordinal of sample 0 (`artificial.trainer_first_ordinal`):
        the batch is a pure function of (seed, ordinal).  weights: uint8 [H0, W0] per sample, per-pixel loss weights that
        follow their label map through the transform; the sample then carries `"target_weight"` (uint8 [B, P*P])."""
        tf = getattr(self, "train_transform", None) or self.build_train_transform()
        if weights is None:
            img, tgt = tf(images, labels, first_ordinal)
        else:
            img, tgt, wgt = tf(images, labels, first_ordinal, weights=weights)
        B, P, dev = len(images), tf.P, tf.device
        src = self._train_src_tokens()
        if src.device != dev:
            src = self._train_src = src.to(dev)
        L = src.numel()
        sample = {
            "id": list(range(B)), "nsentences": B, "ntokens": int(B * (P * P + 1)),
            "net_input": {"src_tokens": src.repeat(B, 1), "src_lengths": torch.full((B,), L, device=dev),
                          "patch_images": img, "patch_masks": torch.ones(B, dtype=torch.bool, device=dev),
                          "prev_output_tokens": torch.zeros(B, 1, dtype=torch.long, device=dev)},
            "target": tgt,
        }
        if weights is not None:
            sample["target_weight"] = wgt
        return sample

    def build_batch_mix(self, mask="class"):
        """The ClassMix / CutMix of two batches (ifseg_amd/augment.py `BatchMix`) with the train transform's patch size,
        class count, seed and device; on a GPU device it runs csrc/mix.hip.  One per mask, kept."""
        from ...augment import BatchMix
        tf = getattr(self, "train_transform", None) or self.build_train_transform()
        mixes = self.__dict__.setdefault("_batch_mixes", {})
        key = (mask, tf.P, tf.nseg, tf.seg_id_offset, tf.seed, tf.device)
        if key not in mixes:
            mixes[key] = BatchMix(tf.P, tf.nseg, tf.seg_id_offset, seed=tf.seed, device=tf.device, mask=mask)
        return mixes[key]

    def mix_samples(self, source_sample, target_sample, first_ordinal, mask="class"):
        """Two batches in `train_sample`'s layout -> one: the pixels of half of the classes present in each source (labelled)
        sample (mask "class", ClassMix) or of a random rectangle (mask "box", CutMix) are pasted over the target
        (pseudo-labelled) sample -- image, label and loss weight travel together (`augment.BatchMix` states the rule; a pure
        function of (seed, first_ordinal + b)).  -> the batch `Trainer.train_step` takes: the target sample with
        `patch_images`, `target` and, if either sample has one, `target_weight` replaced (a missing plane counts as 255).
        A different B, P or prompt length: ValueError."""
        from ...augment import check_mix_batches, mix_batch
        mix = self.build_batch_mix(mask)
        src, dst = mix_batch(source_sample), mix_batch(target_sample)
        check_mix_batches(*src, *dst, what="mix_samples")
        s_tok, d_tok = source_sample["net_input"]["src_tokens"], target_sample["net_input"]["src_tokens"]
        if tuple(s_tok.shape) != tuple(d_tok.shape):
            raise ValueError("mix_samples: the two samples carry prompts of different lengths, %s and %s"
                             % (tuple(s_tok.shape), tuple(d_tok.shape)))
        img, tgt, wgt = mix(src, dst, first_ordinal)
        sample = {k: v for k, v in target_sample.items() if k != "target_weight"}
        sample["net_input"] = dict(target_sample["net_input"], patch_images=img)
        sample["target"] = tgt
        if wgt is not None:
            sample["target_weight"] = wgt
        return sample

    def build_strong_augment(self, **kw):
        """The strong augmentation of a mixed batch (ifseg_amd/augment.py `StrongAugment`: colour jitter, then Gaussian blur)
        with the train transform's patch size, normalisation, channel order, seed and device; on a GPU device it runs
        csrc/strong.hip.  kw: `jitter_p8`, `blur_p8`.  One per key, kept."""
        from ...augment import StrongAugment
        tf = getattr(self, "train_transform", None) or self.build_train_transform()
        augs = self.__dict__.setdefault("_strong_augments", {})
        key = (tf.P, tf.mean, tf.std, tf.reverse_channels, tf.seed, tf.device, tuple(sorted(kw.items())))
        if key not in augs:
            augs[key] = StrongAugment(tf.P, tf.mean, tf.std, seed=tf.seed, device=tf.device, reverse_channels=tf.reverse_channels, **kw)
        return augs[key]

    def strong_augment(self, sample, first_ordinal, **kw):
        """A batch in `train_sample`'s layout -> the same batch with `patch_images` jittered and blurred
        (`augment.StrongAugment` states the rule; a pure function of (seed, first_ordinal + b), on slots of the stream that
        neither the transform nor the mix draws from).  Target, weight plane and prompt are the sample's own tensors."""
        aug = self.build_strong_augment(**kw)
        out = dict(sample)
        out["net_input"] = dict(sample["net_input"], patch_images=aug(sample["net_input"]["patch_images"], first_ordinal))
        return out

    def dacs_sample(self, model, images, labels, unlabeled, first_ordinal, trainer=None, mask="class", strong=False, **kw):
        """One batch of cross-domain mixed self-training (DACS, Tranheden et al. 2021; ClassMix / CutMix): the labelled batch
        `train_sample(images, labels, first_ordinal)` pasted by `mix_samples(..., first_ordinal)` over the pseudo-labelled
        batch `self_train_sample(model, unlabeled, first_ordinal + 2**31, trainer=trainer, confidence_weight=True, **kw)`.
        The unlabelled samples take their ordinals from the upper half of the ordinal range, so the two transforms draw
        independently: first_ordinal + B <= 2**31, else ValueError.  Pasted labelled pixels weigh 255, the rest the teacher's
        confidence; the criterion's default `weight_norm="weights"` is scale-free.  DACS applies a colour jitter and a
        Gaussian blur after the mix: `strong=True` sends the mixed images through `strong_augment(sample, first_ordinal)`;
        by default each half keeps its own transform's jitter and nothing more.  `min_region=K` and `region_connectivity` in
        `kw` reach `pseudo_label_raw` through `self_train_sample`: the small regions leave the pseudo-labelled half before
        the mix."""
        images = [images] if torch.is_tensor(images) else list(images)
        first = int(first_ordinal)
        if first < 0 or first + len(images) > 2 ** 31:
            raise ValueError("dacs_sample: first_ordinal + B must stay within 2**31 (the unlabelled batch draws at "
                             "first_ordinal + 2**31), got %d + %d" % (first, len(images)))
        source = self.train_sample(images, labels, first)
        target = self.self_train_sample(model, unlabeled, first + 2 ** 31, trainer=trainer, confidence_weight=True, **kw)
        sample = self.mix_samples(source, target, first, mask=mask)
        return self.strong_augment(sample, first) if strong else sample

    def train_step(self, sample, model, criterion, optimizer, update_num, ignore_grad=False, **extra_kwargs):
        """tasks/mm_tasks/segmentation.py:190-222."""
        if not model.training:      # nn.Module.train() walks every sub-module: only when the mode changes
            model.train()
        model.set_num_updates(update_num)
        loss, sample_size, logging_output = criterion(model, sample, update_num=update_num,
                                                      ema_model=extra_kwargs.get("ema_model"))
        if ignore_grad:
            loss = loss * 0
        if optimizer is not None:
            optimizer.backward(loss)
        else:
            loss.backward()
        return loss, sample_size, logging_output

    def valid_step(self, sample, model, criterion, **extra_kwargs):
        """tasks/mm_tasks/segmentation.py:225-229."""
        if model.training:
            model.eval()
        with torch.no_grad():
            loss, sample_size, logging_output = criterion(model, sample)
        return loss, sample_size, logging_output
