"""HuggingFace surface (drop-in for /root/reference/src/model/language_model/{u2llama,u2qwen3,u2phi3}.py).

`forward(images, input_ids, labels, attention_mask, question_ids, ...)` and
`generate(images, inputs, question_ids=..., **kwargs)` keep the reference's call shapes
(u2llama.py:41-127; eval/mrg.py:74; dpo_u2trainer.py:71-79,267-272).  The decoder itself is stock HF on
PyTorch-ROCm; only `prepare_inputs_for_multimodal` (arch.py) runs the HIP path.
"""
from __future__ import annotations

from typing import Any, List, Optional, Tuple, Union

import torch
import torch.nn as nn
from transformers import (AutoConfig, AutoModelForCausalLM, LlamaConfig, LlamaForCausalLM, LlamaModel, Phi3Config,
                          Phi3ForCausalLM, Phi3Model, Qwen3Config, Qwen3ForCausalLM, Qwen3Model)
from transformers.modeling_outputs import CausalLMOutputWithPast

from .arch import u2MetaForCausalLM, u2MetaModel


class u2Config(LlamaConfig):
    model_type = "u2llama"


class u2Qwen3Config(Qwen3Config):
    model_type = "u2Qwen3"


class u2Phi3Config(Phi3Config):
    model_type = "u2phi3"


class u2LlamaModel(u2MetaModel, LlamaModel):
    config_class = u2Config

    def __init__(self, config: LlamaConfig):
        super(u2LlamaModel, self).__init__(config)


class u2Qwen3Model(u2MetaModel, Qwen3Model):
    config_class = u2Qwen3Config

    def __init__(self, config: Qwen3Config):
        super(u2Qwen3Model, self).__init__(config)


class u2Phi3Model(u2MetaModel, Phi3Model):
    config_class = u2Phi3Config

    def __init__(self, config: Phi3Config):
        super(u2Phi3Model, self).__init__(config)


_ROUTE_ATTRS = {}


def _route_attrs(grad: bool):
    """The config attributes (with their defaults) that ask for the decoder route of a grad mode -- the training route with grad,
    the prefill and decode steps without --, from prefill.SWITCHES: the switch itself and those that imply or need it.  Read once."""
    attrs = _ROUTE_ATTRS.get(grad)
    if attrs is None:
        from .prefill import SWITCHES
        kw = "train" if grad else "prefill"
        attrs = _ROUTE_ATTRS[grad] = tuple((s.config, s.default) for s in SWITCHES
                                           if s.config and (s.kw == kw or kw in s.implies + s.needs))
    return attrs


class _u2CausalLMMixin(u2MetaForCausalLM):
    """forward / generate / prepare_inputs_for_generation shared by the Llama, Qwen3 and Phi3 builds."""

    def get_model(self):
        return self.model

    def _maybe_fuse(self) -> None:
        """Patch the decoder layers for the HIP routes of prefill.py, once per grad mode, when the decoder sits on the GPU in a
        type that mode's route computes: without grad the prefill and decode steps (bf16, or fp16 on the f16
        build), with grad the training route of decoder_train.py (bf16).  The switches are the config attributes of
        prefill.SWITCHES (`config.u2_fused_prefill`, default True; every other one default False), passed on as the config has
        them with what each implies or needs."""
        grad = torch.is_grad_enabled()
        checked = self.__dict__.setdefault("_u2_fuse_checked", set())
        if grad in checked:
            return
        # (nothing below is remembered when it says no -- the config and the device may change --, so the no is cheap: the one to
        #  three config attributes that ask for this mode's route, then the first parameter's device)
        config = self.config
        for attr, default in _route_attrs(grad):
            if getattr(config, attr, default):
                break
        else:
            return
        p = next(self.model.layers[0].parameters(), None) if len(self.model.layers) else None
        if p is None or not p.is_cuda:
            return
        from . import prefill
        if p.dtype in (prefill.TRAIN_DTYPES if grad else prefill.INFER_DTYPES):
            on = {s.kw: bool(getattr(config, s.config, s.default)) for s in prefill.SWITCHES if s.config}
            for s in prefill.SWITCHES:
                if on.get(s.kw):
                    on.update(dict.fromkeys(s.implies + s.needs, True))
            defaults = {s.kw: s.default for s in prefill.SWITCHES}
            prefill.enable_fused_prefill(self, strict=False, **{k: v for k, v in on.items() if v != defaults[k]})
            checked.add(grad)

    def _loss_head_ok(self, kwargs=None) -> bool:
        """Whether a call with labels takes the loss head of loss_head.py (`config.u2_fused_loss_head`, default False) instead
        of lm_head + ForCausalLMLoss: lm_head exactly nn.Linear, no bias, no hooks (a LoRA-wrapped or probed head keeps the stock
        path, as prefill._admit has it for the layers), bf16 on the GPU in a shape the head computes, the stock causal-LM
        loss, all positions scored (no `logits_to_keep`) and a ModelOutput asked for.  On that route
        `config.u2_fused_loss_head_predictions` (default False) puts the positions' argmax where the logits would be."""
        if not bool(getattr(self.config, "u2_fused_loss_head", False)):
            return False
        kwargs = kwargs or {}
        keep = kwargs.get("logits_to_keep", 0)
        if not (keep is None or (isinstance(keep, int) and keep == 0)) or kwargs.get("return_dict", True) is False:
            return False
        from transformers.loss.loss_utils import ForCausalLMLoss
        return self._plain_lm_head() and self.loss_function is ForCausalLMLoss

    def _plain_lm_head(self) -> bool:
        """lm_head is exactly nn.Linear without bias or hooks, bf16 on the GPU, in a shape the loss head computes: reading its
        `.weight` instead of calling it is then the same computation."""
        from .loss_head import supported
        from .lora import _HOOK_TABLES
        head = self.lm_head
        return (type(head) is nn.Linear and head.bias is None and not any(getattr(head, t, None) for t in _HOOK_TABLES)
                and head.weight.is_cuda and supported(head.in_features, head.out_features, head.weight.dtype))

    def token_logprobs(self, images: Optional[torch.Tensor], input_ids: torch.LongTensor, labels: torch.LongTensor,
                       attention_mask: Optional[torch.Tensor] = None, question_ids: Optional[torch.LongTensor] = None,
                       **kwargs) -> torch.Tensor:
        """log p(label) of every position, (B, S) fp32, 0 where the label is -100: the multimodal preparation, the decoder, then
        the loss head on the labels as `prepare_inputs_for_multimodal` returns them (shifted by one inside) -- what a DPO trainer
        takes from the policy (with grad) and from the reference model (under no_grad) as gather(log_softmax(logits)) * mask
        (dpo_u2trainer.py:295-309), without the logits.  The head must qualify (_plain_lm_head; the config switch is not
        needed): there is no fallback."""
        from . import loss_head
        self._maybe_fuse()
        if not self._plain_lm_head():
            raise RuntimeError("token_logprobs: needs a plain nn.Linear lm_head (no bias, hooks or adapters), bf16 on the GPU, with "
                               "vocab % 8 == 0 and hidden % 64 == 0")
        (input_ids, position_ids, attention_mask, _, inputs_embeds, labels) = self.prepare_inputs_for_multimodal(
            input_ids, None, attention_mask, None, labels, images, question_ids)
        hidden = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                            inputs_embeds=inputs_embeds, use_cache=False, **kwargs).last_hidden_state
        return loss_head.token_logprobs(hidden, self.lm_head.weight, labels)

    def token_stats(self, images: Optional[torch.Tensor], input_ids: torch.LongTensor, labels: torch.LongTensor,
                    attention_mask: Optional[torch.Tensor] = None, question_ids: Optional[torch.LongTensor] = None,
                    want=(), **kwargs):
        """`token_logprobs` with the further per-position statistics of the logits named in `want` ("argmax", "logit_sum",
        "lse2"), all from the one walk over the vocabulary: a loss_head.TokenStats, (B, S) each, whose `logprob` is
        `token_logprobs`' result.  With want=("logit_sum", "lse2") it carries everything a DPO trainer's concatenated forward
        reads from the logits (loss_head.dpo_outputs).  The same preparation and the same rule: the head must qualify
        (_plain_lm_head), there is no fallback."""
        from . import loss_head
        self._maybe_fuse()
        if not self._plain_lm_head():
            raise RuntimeError("token_stats: needs a plain nn.Linear lm_head (no bias, hooks or adapters), bf16 on the GPU, with "
                               "vocab % 8 == 0 and hidden % 64 == 0")
        (input_ids, position_ids, attention_mask, _, inputs_embeds, labels) = self.prepare_inputs_for_multimodal(
            input_ids, None, attention_mask, None, labels, images, question_ids)
        hidden = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                            inputs_embeds=inputs_embeds, use_cache=False, **kwargs).last_hidden_state
        return loss_head.token_stats(hidden, self.lm_head.weight, labels, want=want)

    def forward(self, images: Optional[torch.FloatTensor] = None, input_ids: torch.LongTensor = None,
                labels: Optional[torch.LongTensor] = None, attention_mask: Optional[torch.Tensor] = None,
                question_ids: Optional[torch.LongTensor] = None, position_ids: Optional[torch.LongTensor] = None,
                past_key_values: Optional[List[torch.FloatTensor]] = None,
                inputs_embeds: Optional[torch.FloatTensor] = None, use_cache: Optional[bool] = None,
                output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, **kwargs) -> Union[Tuple, CausalLMOutputWithPast]:
        # aliases used by the in-tree Qwen3 variant (u2qwen3.py:42-47)
        images = kwargs.pop("vision_input", images)
        question_ids = kwargs.pop("raw_question_ids", question_ids)
        self._maybe_fuse()
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = \
                self.prepare_inputs_for_multimodal(input_ids, position_ids, attention_mask, past_key_values, labels,
                                                   images, question_ids)
        for k, v in (("output_attentions", output_attentions), ("output_hidden_states", output_hidden_states),
                     ("return_dict", return_dict)):
            if v is not None:
                kwargs[k] = v
        if labels is not None and self._loss_head_ok(kwargs):
            from . import loss_head
            outputs = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=past_key_values, inputs_embeds=inputs_embeds, use_cache=use_cache, **kwargs)
            shifted = kwargs.get("shift_labels")
            predictions = None
            if bool(getattr(self.config, "u2_fused_loss_head_predictions", False)):
                # (default False) the output's `logits` = the (B, S) int64 argmax of every scored position, from the same walk:
                # position t holds the prediction for label t + 1, `ignore_index` where that label is ignored -- what an SFT
                # evaluation compares as predictions[:, :-1] against labels[:, 1:] (loss_head.predictions_for_metrics)
                st = loss_head.token_stats(
                    outputs.last_hidden_state, self.lm_head.weight, labels if shifted is None else shifted, want=("argmax",),
                    ignore_index=kwargs.get("ignore_index", -100), shift=shifted is None)
                loss = loss_head.reduce_nll(-st.logprob, st.labelled, kwargs.get("num_items_in_batch"))
                predictions = st.argmax
            else:
                loss = loss_head.linear_cross_entropy(
                    outputs.last_hidden_state, self.lm_head.weight, labels if shifted is None else shifted,
                    ignore_index=kwargs.get("ignore_index", -100), num_items_in_batch=kwargs.get("num_items_in_batch"),
                    shift=shifted is None)
            return CausalLMOutputWithPast(loss=loss, logits=predictions, past_key_values=outputs.past_key_values,
                                          hidden_states=outputs.hidden_states, attentions=outputs.attentions)
        if "_u2_stack" in self.model.__dict__:
            # `config.u2_fused_decode_head` (default False): a decode step without labels that the whole-stack route admits runs
            # its head in the same library call (prefill.head_route: final norm, lm_head in `config.u2_fused_head_form`, logits
            # (B, 1, V) fp32); every other call goes on below as it came
            from . import prefill
            out = prefill.head_forward(self, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache,
                                       labels, kwargs)
            if out is not None:
                return out
        return super().forward(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                               past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels,
                               use_cache=use_cache, **kwargs)

    def _get_logits_processor(self, *args, **kwargs):
        """transformers' processor list; with `config.u2_fused_sampling` (default False) its temperature / top-k / top-p run becomes one
        FusedSamplingWarper (sampling.py: one HIP launch, no sort; beam sampling's min_tokens_to_keep = 2 included).  With the switch off
        the list is returned untouched.  `config.u2_fused_sampling_split` (default False, read only with the first): calls of at most
        sampling.SPLIT_MAX_ROWS rows take the split-row form of the kernel (the same bits)."""
        processors = super()._get_logits_processor(*args, **kwargs)
        if bool(getattr(self.config, "u2_fused_sampling", False)):
            from .sampling import fuse_warpers
            processors = fuse_warpers(processors, split=bool(getattr(self.config, "u2_fused_sampling_split", False)))
        return processors

    @torch.no_grad()
    def generate(self, images: Optional[torch.Tensor] = None, inputs: Optional[torch.Tensor] = None,
                 question_ids: Optional[torch.Tensor] = None, **kwargs) -> Any:
        position_ids = kwargs.pop("position_ids", None)
        attention_mask = kwargs.pop("attention_mask", None)
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported")
        if images is not None:
            (inputs, position_ids, attention_mask, _, inputs_embeds, _) = self.prepare_inputs_for_multimodal(
                inputs, position_ids, attention_mask, None, None, images, question_ids)
        else:
            inputs_embeds = self.get_model().embed_tokens(inputs)
        return super().generate(inputs_embeds=inputs_embeds, **kwargs)

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, **kwargs):
        images = kwargs.pop("images", None)
        inputs = super().prepare_inputs_for_generation(input_ids, past_key_values=past_key_values,
                                                       inputs_embeds=inputs_embeds, **kwargs)
        if images is not None:
            inputs["images"] = images
        return inputs


class u2LlamaForCausalLM(_u2CausalLMMixin, LlamaForCausalLM):
    config_class = u2Config

    def __init__(self, config):
        super(LlamaForCausalLM, self).__init__(config)
        self.model = u2LlamaModel(config)
        self.pretraining_tp = getattr(config, "pretraining_tp", 1)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.post_init()


class u2Qwen3ForCausalLM(_u2CausalLMMixin, Qwen3ForCausalLM):
    config_class = u2Qwen3Config

    def __init__(self, config):
        super(Qwen3ForCausalLM, self).__init__(config)
        self.model = u2Qwen3Model(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.post_init()


class u2Phi3ForCausalLM(_u2CausalLMMixin, Phi3ForCausalLM):
    """language_model/u2phi3.py:25-140 (train_stage1.py:290-296, model_type "phi3").  The path in front of the decoder is the
    same HIP path; the Phi-3 decoder layers (packed qkv_proj / gate_up_proj modules, used as they are) take the fused prefill
    and decode steps of prefill.py like the other two builds, behind the same `config.u2_fused_prefill` switch: head dim
    96 (Phi-3-mini) or 64 / 128, SiLU, rotary over the whole head.  With `sliding_window` = W a prefill of more than W
    positions takes the stock layers; decode steps attend over the last W positions.  `config.u2_fused_phi3_training = True`
    (default False) trains the layers on the route of decoder_train.py (calls of S <= W positions)."""
    config_class = u2Phi3Config

    def __init__(self, config):
        super(Phi3ForCausalLM, self).__init__(config)
        self.model = u2Phi3Model(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.post_init()


def register_auto_classes() -> None:
    """AutoConfig/AutoModelForCausalLM registration (u2llama.py:141-142, u2qwen3.py:144-145, u2phi3.py:139-140); idempotent."""
    for cfg, cls in ((u2Config, u2LlamaForCausalLM), (u2Qwen3Config, u2Qwen3ForCausalLM), (u2Phi3Config, u2Phi3ForCausalLM)):
        try:
            AutoConfig.register(cfg.model_type, cfg)
            AutoModelForCausalLM.register(cfg, cls)
        except ValueError:
            pass  # already registered (e.g. the reference package was imported first)


register_auto_classes()
