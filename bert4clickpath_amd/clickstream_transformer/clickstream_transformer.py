"""ClickstreamTransformer: the drop-in model surface (reference
clickstream_transformer/clickstream_transformer.py:8-375), MI355X-native.

Differences forced by the platform, all at the edge:
  * PyTorch has no string tensors.  Each input feature may be a nested list / numpy array of ``str``
    (looked up on the host exactly as the reference's StaticVocabularyTable: 10 reserved tokens +
    vocabulary file, one OOV bucket) or an int64 tensor of already looked-up ids (no specials).
  * ``cloze_loss`` / ``predict_topk`` are the fused training / ranking entry points: same numbers as
    ``head(...)`` followed by ClozeMaskedLoss / top_k, without materialising (B*M) x V probabilities.
"""
import numpy as np
import torch
from torch import nn

from .. import ops
from .._lib import CE_PLAIN, CE_TF, B4CError
from .constants import CLS, INPUT_PAD, MASK_ID, RESERVED_TOKENS, SEP, CLASSIFICATION_TOKEN, SEPARATOR_TOKEN
from .training_utils import load_vocabulary
from .transformer import Transformer


def _is_string_feature(x):
    if isinstance(x, torch.Tensor):
        return False
    a = np.asarray(x)
    return a.dtype.kind in ('U', 'S', 'O')


class TransformerInputPrep:
    """[CLS] [SEP] seq_1 [SEP] seq_2 [SEP] ... per chained feature (reference :8-103)."""

    _special_cols = {}

    def __init__(self, seq_chain_mapping):
        self.seq_chain_mapping = seq_chain_mapping

    @staticmethod
    def _chain_sequences(sequences):
        # (a nested list without any element -- a (B, 0) sequence -- has no dtype of its own: the chain is of strings as soon
        # as ONE of its sequences is, and of int64 ids when none says otherwise)
        if any(_is_string_feature(x) for x in sequences):
            seqs = [np.asarray(s, dtype=object) for s in sequences]
            B = seqs[0].shape[0]
            cls = np.full((B, 1), CLASSIFICATION_TOKEN, dtype=object)
            sep = np.full((B, 1), SEPARATOR_TOKEN, dtype=object)
            parts = [cls, sep]
            for s in seqs:
                parts += [s.reshape(B, -1), sep]
            return np.concatenate(parts, axis=1)
        seqs = [s if isinstance(s, torch.Tensor) else torch.as_tensor(np.asarray(s).astype(np.int64) if np.asarray(s).size == 0 else s)
                for s in sequences]
        B = seqs[0].shape[0]
        if all(s.is_cuda and s.dtype == torch.int64 and s.dim() == 2 for s in seqs) and len(seqs) <= 8:
            return ops.chain_ids(seqs, CLS, SEP)          # one library launch instead of torch.cat
        key = (B, seqs[0].dtype, seqs[0].device)
        cols = TransformerInputPrep._special_cols.get(key)
        if cols is None:            # the [CLS] / [SEP] columns of a batch size are constants: built once, not every step
            if len(TransformerInputPrep._special_cols) > 64:
                TransformerInputPrep._special_cols.clear()
            cols = (torch.full((B, 1), CLS, dtype=seqs[0].dtype, device=seqs[0].device),
                    torch.full((B, 1), SEP, dtype=seqs[0].dtype, device=seqs[0].device))
            TransformerInputPrep._special_cols[key] = cols
        cls, sep = cols
        parts = [cls, sep]
        for s in seqs:
            parts += [s, sep]
        return torch.cat(parts, dim=1)

    def __call__(self, features, keep_features=False):
        features = dict(features)
        lens = None
        for new_feature, names in self.seq_chain_mapping.items():
            seqs = [features[n] for n in names]
            features[new_feature] = self._chain_sequences(seqs)
            if lens is None:
                lens = [int(np.asarray(s).shape[1]) if not isinstance(s, torch.Tensor) else int(s.shape[1]) for s in seqs]
        first = features[list(self.seq_chain_mapping.keys())[0]]
        if isinstance(first, np.ndarray) and first.dtype == object and first.shape[0] > 0:
            # the reference's rule, literally (:79-90): every position of ROW 0 that holds '[SEP]' ends a segment -- also an
            # item that happens to be that token
            ends = [int(i) for i in np.flatnonzero(first[0] == SEPARATOR_TOKEN)]
        else:
            # integer ids (possibly on the GPU: no read-back): the separators sit where the chain put them, the same in every row
            ends, pos = [1], 1
            for n in lens:
                pos += n + 1
                ends.append(pos)
        starts = [0] + [e + 1 for e in ends[:-1]]
        if not keep_features:
            drop = set()
            for names in self.seq_chain_mapping.values():
                drop |= set(names)
            features = {k: v for k, v in features.items() if k not in drop}
        return features, starts, ends


class ClickstreamTransformer(nn.Module):
    def __init__(self, sequential_input_config, feature_vocabs, embedding_dims, head_unit, segment_to_head=None,
                 value_to_head=None, num_encoder_layers=1, num_attention_heads=1, dropout_rate=0.1,
                 compute_dtype=torch.float32, feature_combine='concat', encoder_ff_dim=100, ffn_activation='relu',
                 position_encoding='sinusoidal', max_positions=None, attention_dropout_rate=0.0, embedding_layernorm=False,
                 embedding_scale=None, attention='bidirectional', norm='post', **kwargs):
        super().__init__()
        # ffn_activation / position_encoding / max_positions: the BERT4Rec paper's GELU feed-forward and learned positions
        # (extensions, validated by transformer.Transformer); the defaults are the reference's ReLU and fixed sinusoid
        self.ffn_activation, self.position_encoding = ffn_activation, position_encoding
        # attention_dropout_rate: dropout on the attention probabilities in training (BERT's attention_probs_dropout_prob, 0.2 in
        # the published BERT4Rec configurations); the reference's attention has none, the default 0 is the reference's
        self.attention_dropout_rate = float(attention_dropout_rate)
        # encoder_ff_dim: the reference hard-codes the FFN width 100 in this constructor (:225) and takes it as an argument of the
        # inner API (transformer.Transformer); 4 * d_model is the BERT4Rec paper's width.  Default = the reference's.
        self.encoder_ff_dim = int(encoder_ff_dim)
        self.feature_combine = feature_combine      # 'sum': the features' embedding rows are added (extension, transformer.Transformer)
        self.sequential_input_config = sequential_input_config
        self.feature_vocabs = feature_vocabs
        self.embedding_dims = embedding_dims
        self.head = head_unit
        self.num_encoder_layers, self.num_attention_heads, self.dropout_rate = \
            num_encoder_layers, num_attention_heads, dropout_rate
        assert (segment_to_head is not None or value_to_head is not None) and \
               (segment_to_head is None or value_to_head is None), \
               "Exactly one of segment_to_head and value_to_head must be provided."
        self.segment_to_head, self.value_to_head = segment_to_head, value_to_head
        self.transformer_input_prep = TransformerInputPrep(self.sequential_input_config)
        self.vocab_lookup_tables = self._create_lookup_tables(self.feature_vocabs, RESERVED_TOKENS)
        # KeyError if a feature is embedded but has no vocabulary, as in the reference (:212-217)
        self.embedding_sizes = {f: self.vocab_lookup_tables[f]['size'] for f in self.feature_vocabs.keys()}
        self.transformer = Transformer(
            embedding_sizes={f: self.embedding_sizes[f] for f in self.embedding_dims.keys()},
            embedding_dims=self.embedding_dims, num_layers=num_encoder_layers,
            num_attention_heads=num_attention_heads, encoder_ff_dim=self.encoder_ff_dim,   # 100: hard-coded in the reference (:225)
            dropout_rate=dropout_rate, compute_dtype=compute_dtype, feature_combine=feature_combine,
            ffn_activation=ffn_activation, position_encoding=position_encoding, max_positions=max_positions,
            attention_dropout_rate=attention_dropout_rate, embedding_layernorm=embedding_layernorm,
            embedding_scale=embedding_scale, attention=attention, **({'norm': norm} if norm != 'post' else {}))
        # norm: 'post' (the reference) | 'pre' (pre-LN layers and a final LayerNorm, transformer.Encoder; validated by
        # transformer.Transformer).  A pre-LN encoder evaluates its full last layer (no masked-query form).
        self.norm = self.transformer.norm
        self.max_positions = self.transformer.max_positions
        # attention: 'bidirectional' (the reference, BERT4Rec) | 'causal' (left-to-right: SASRec, the paper's unidirectional arm;
        # validated by transformer.Transformer).  A causal encoder evaluates its full last layer (no masked-query form).
        self.attention = self.transformer.attention
        # embedding_layernorm / embedding_scale: the paper's input stage drop(LayerNorm(E + P)) (transformer.Transformer)
        self.embedding_layernorm, self.embedding_scale = self.transformer.embedding_layernorm, self.transformer.embedding_scale
        if hasattr(self.head, 'tie') and getattr(self.head, '_table', None) is None:
            # tied-weight head: project back onto the FIRST embedded feature's table (the items)
            first = list(self.embedding_dims.keys())[0]
            self.head.tie(self.transformer.embedding_layers[first].weight)
        if hasattr(self.head, 'build'):
            self.head.build(self.transformer.d_model)

    @property
    def compute_dtype(self):
        return self.transformer.compute_dtype

    def set_compute_dtype(self, dtype):
        self.transformer.compute_dtype = dtype
        return self

    def get_config(self):
        return {'sequential_input_config': self.sequential_input_config, 'feature_vocabs': self.feature_vocabs,
                'embedding_dims': self.embedding_dims, 'head_unit': self.head, 'segment_to_head': self.segment_to_head,
                'value_to_head': self.value_to_head, 'num_encoder_layers': self.num_encoder_layers,
                'num_attention_heads': self.num_attention_heads, 'dropout_rate': self.dropout_rate,
                **({'feature_combine': 'sum'} if self.feature_combine == 'sum' else {}),
                **({'encoder_ff_dim': self.encoder_ff_dim} if self.encoder_ff_dim != 100 else {}),
                **({'ffn_activation': self.ffn_activation} if self.ffn_activation != 'relu' else {}),
                **({'position_encoding': 'learned', 'max_positions': self.max_positions}
                   if self.position_encoding == 'learned' else {}),
                **({'attention_dropout_rate': self.attention_dropout_rate} if self.attention_dropout_rate else {}),
                **({'embedding_layernorm': True} if self.embedding_layernorm else {}),
                **({'embedding_scale': self.embedding_scale} if self.embedding_scale is not None else {}),
                **({'attention': self.attention} if self.attention != 'bidirectional' else {}),
                **({'norm': self.norm} if self.norm != 'post' else {})}

    @staticmethod
    def _create_lookup_tables(vocabularies, tokens_to_prepend=None):
        """token -> id over [reserved tokens] + vocabulary lines; one OOV bucket id == len(keys);
        table size == len(keys) + 1 (reference :247-258, :217)."""
        tables = {}
        for feature_name, vocab_file in vocabularies.items():
            keys = load_vocabulary(vocab_file) if isinstance(vocab_file, str) else [str(t).strip() for t in vocab_file]
            if tokens_to_prepend is not None:
                keys = list(tokens_to_prepend) + list(keys)
            table = {}
            for i, k in enumerate(keys):
                table.setdefault(k, i)
            tables[feature_name] = {'table': table, 'oov': len(keys), 'size': len(keys) + 1}
        return tables

    def lookup(self, feature_name, tokens):
        t = self.vocab_lookup_tables[feature_name]
        table, oov = t['table'], t['oov']
        a = np.asarray(tokens, dtype=object)
        flat = np.fromiter((table.get(x if isinstance(x, str) else x.decode(), oov) for x in a.reshape(-1)),
                           dtype=np.int64, count=a.size)
        return flat.reshape(a.shape)

    # ---- shared front half: chain, look up, encode -------------------------------------------
    def _encode(self, inputs, training, pack=False, n_real_tokens=None, rows_of=None):
        """rows_of(ids_first, raw_first) -> (flat_idx, offsets, extra) or None: called once the ids are known; when it returns
        indices, the last encoder layer is evaluated at those positions only and `enc` is the (R, d) rows."""
        raw_features, seg_starts, seg_ends = self.transformer_input_prep(features=inputs)
        dev = self.transformer.position_table.device
        if dev.type != 'cuda':
            raise B4CError('model is on %s: move it to the HIP device with .to("cuda") (no CPU path)' % dev)
        features = dict(raw_features)
        for name in self.vocab_lookup_tables.keys():
            if name not in features:
                continue
            x = features[name]
            if _is_string_feature(x):
                x = torch.from_numpy(self.lookup(name, x))
            features[name] = torch.as_tensor(x).to(device=dev, dtype=torch.int64)
        seq = {name: features[name] for name in self.sequential_input_config.keys()}
        first = list(self.sequential_input_config.keys())[0]
        self._packed = None
        if pack:
            # padding-free layout: the encoder runs on the real tokens only (pad keys are masked, pad queries are never read,
            # their gradient under the Cloze loss is exactly zero -- include/b4c.h "packed token layout")
            ids0 = seq[first].contiguous()
            B, S = ids0.shape
            cap = int(n_real_tokens) if n_real_tokens is not None else B * S
            counts, cu, tok_src, packed_of, mx = ops.nonpad_positions(ids0, cap)
            if n_real_tokens is not None:
                T_real = cap                      # the caller's count avoids the read-back
            else:
                T_real = int(counts.sum().item())
                if T_real != cap:                 # (every position real is the only case where they agree)
                    counts, cu, tok_src, packed_of, mx = ops.nonpad_positions(ids0, T_real)
            self._packed = ops.Packed(cu, tok_src, packed_of, B, S, T_real, S)
            self._packed.ids_packed = mx          # < 0: the given n_real_tokens was wrong (poisons the loss, see cloze_loss)
        rows = None
        self._rows_extra = None
        if rows_of is not None:
            got = rows_of(seq[first], raw_features[first])
            if got is not None:
                flat_idx, offsets, self._rows_extra = got
                if self._packed is not None:
                    flat_idx = ops.remap_index(flat_idx.contiguous(), self._packed.packed_of)
                rows = (flat_idx.contiguous(), offsets.contiguous())
        enc, key_pad = self.transformer(seq, training, None, return_key_pad=True, packed=self._packed, rows=rows)
        return enc, seq[first], raw_features[first], seg_starts, seg_ends

    def _use_packed(self, inputs, packed, n_real_tokens):
        """packed=None: use the padding-free layout when the caller supplies the real-token count (no read-back needed);
        True: always (one device read-back for the count when it is not given); False: dense."""
        if packed is False or self.value_to_head is None:
            return False
        if packed is None and n_real_tokens is None:
            return False
        first_in = self.sequential_input_config[list(self.sequential_input_config.keys())[0]]
        S = sum((inputs[n].shape[1] if isinstance(inputs[n], torch.Tensor) else np.asarray(inputs[n], dtype=object).shape[1])
                for n in first_in) + len(first_in) + 2
        ok = self.transformer.packed_supported(S)
        if packed is True and not ok:
            raise B4CError('packed=True needs bf16 compute, head depth 32 / 64 and an encoder length <= %s'
                           % ('%d' % ops.ATTN_LONG_MAX_S if ops.long_attn else '512'))
        return ok

    def _match_positions(self, ids_first, raw_first, cap=None, poison=None):
        """Flat (b*S+s) indices, row-major, where the first feature's RAW value == value_to_head.  More matches than `cap`:
        offsets clamped to cap, the returned maxcount negative and the int32 flag `poison` set to -1 (ops.mask_positions)."""
        name = list(self.sequential_input_config.keys())[0]
        t = self.vocab_lookup_tables[name]
        vid = t['table'].get(self.value_to_head, t['oov'])
        if vid == t['oov'] and _is_string_feature(raw_first):
            # value_to_head is not a vocabulary entry: ids cannot tell it from other OOV tokens,
            # so match the raw strings on the host (index generation only).
            hit = (np.asarray(raw_first, dtype=object) == self.value_to_head)
            ids_first = torch.from_numpy(np.where(hit, -7, 0).astype(np.int64)).to(ids_first.device)
            vid = -7
        return ops.mask_positions(ids_first.contiguous(), int(vid), cap, poison)

    def _poisoned(self, out, n_real_tokens):
        """forward() with a caller-given n_real_tokens: a count that disagrees with the device's own would silently drop
        tokens or invent token-0 rows.  The head's output is overwritten with NaN when the device flag says so (a kernel
        that returns at once otherwise), without a read-back.  (The flag goes to the OUTPUT: a NaN in the head's input
        would not survive its ReLUs.)"""
        if self._packed is None or n_real_tokens is None or not isinstance(out, torch.Tensor) or not out.is_floating_point():
            return out
        return ops.poison_rows(out, self._packed.ids_packed)

    # ---- reference call ------------------------------------------------------------------------
    def forward(self, inputs, training=None, mask=None, max_matches=None, packed=None, n_real_tokens=None, scores=None):
        """inputs: dict feature-name -> (B, Li) strings or int64 ids (+ optional 'instance_id').
        Returns head_unit(head_input), or {'instance_id', 'logits'} when 'instance_id' is present.
        packed / n_real_tokens: as in cloze_loss (value_to_head models only).
        scores='lazy' (scoring only, value_to_head models): the head's (B, M, V) output as a head.ClozeScores -- the rows the
        projection would be applied to, not its result; cloze.ClozeMaskedRecall / NDCG rank through it without the scores
        ever reaching memory, `.probabilities()` materialises them.  Heads without that form return their usual output."""
        self._lazy = scores == 'lazy' and hasattr(self.head, 'lazy_scores') and not (training and torch.is_grad_enabled())
        try:
            return self._forward(inputs, training, mask, max_matches, packed, n_real_tokens)
        finally:
            self._lazy = False

    def _head_out(self, head_input, n_real_tokens):
        if self._lazy:
            out = self.head.lazy_scores(head_input)
            if out is not None:
                if self._packed is not None and n_real_tokens is not None:
                    out.flag = self._packed.ids_packed
                return out
        return self._poisoned(self.head(head_input), n_real_tokens)

    def _forward(self, inputs, training, mask, max_matches, packed, n_real_tokens):
        feats = {k: v for k, v in inputs.items() if k != 'instance_id'}
        pack = self._use_packed(feats, packed, n_real_tokens)
        if self.segment_to_head is None and self.value_to_head is not None and ops.mq_last_layer and \
                self.transformer.encoder.rows_route(None, training):
            # the head reads the rows at the value_to_head positions only: the last encoder layer is evaluated for those
            # rows alone (padded to M per sequence; a padding slot is a query row made of zeros whose output nobody reads)
            def positions(ids_first, raw_first):
                counts, offsets, flat, mx = self._match_positions(ids_first, raw_first)
                M = int(mx.item()) if max_matches is None else int(max_matches)   # .item(): the padded width
                if M == 0:
                    return None
                B = ids_first.shape[0]
                pidx = ops.padded_index(counts, offsets, flat, B, M)
                moff = torch.arange(B + 1, dtype=torch.int32, device=pidx.device) * M
                # the reference pads the (B, M, d) head input with ZERO rows (ragged -> dense): slot i keeps its row, a padding
                # slot gathers row -1 = zeros
                keep = torch.where(pidx >= 0, torch.arange(B * M, dtype=torch.int32, device=pidx.device),
                                   torch.full_like(pidx, -1))
                return pidx, moff, (M, keep)
            enc, ids_first, raw_first, seg_starts, seg_ends = self._encode(feats, training, pack, n_real_tokens, rows_of=positions)
            if self._rows_extra is not None:
                M, keep = self._rows_extra
                B = ids_first.shape[0]
                enc = ops.GatherRowsFn.apply(enc, keep, B * M)
                logits = self._head_out(enc.view(B, M, enc.shape[-1]), n_real_tokens)
                if 'instance_id' in inputs.keys():
                    return {'instance_id': inputs['instance_id'], 'logits': logits}
                return logits
            head_input = enc.new_zeros(ids_first.shape[0], 0, enc.shape[-1])       # no position matches anywhere
            logits = self._head_out(head_input, n_real_tokens)
            if 'instance_id' in inputs.keys():
                return {'instance_id': inputs['instance_id'], 'logits': logits}
            return logits
        enc, ids_first, raw_first, seg_starts, seg_ends = self._encode(feats, training, pack, n_real_tokens)
        B, S = ids_first.shape
        d = enc.shape[-1]
        if self.segment_to_head is not None:
            head_input = enc[:, seg_starts[self.segment_to_head]:seg_ends[self.segment_to_head], :].contiguous()
        elif self.value_to_head is not None:
            counts, offsets, flat, mx = self._match_positions(ids_first, raw_first)
            M = int(mx.item()) if max_matches is None else int(max_matches)   # .item(): the padded width
            if M == 0:
                head_input = enc.new_zeros(B, 0, d)
            else:
                pidx = ops.padded_index(counts, offsets, flat, B, M)
                if self._packed is not None:
                    pidx = ops.remap_index(pidx, self._packed.packed_of)
                head_input = ops.GatherRowsFn.apply(enc.reshape(-1, d), pidx, B * M).view(B, M, d)
        else:
            raise ValueError("One of value_to_head and segment_to_head must be provided.")
        logits = self._head_out(head_input, n_real_tokens)
        if 'instance_id' in inputs.keys():
            return {'instance_id': inputs['instance_id'], 'logits': logits}
        return logits

    # ---- fused MI355X entry points ----------------------------------------------------------------
    def _masked_rows(self, inputs, training, flat_idx=None, cap=None, labels_padded=None, pack=False, n_real_tokens=None,
                     row_offsets=None):
        """Encoder output rows at the [MASK] positions, row-major.
        flat_idx given: used as is (a callable: called with the first chain's (B, S) ids once they are on the device, returns the
        indices); with row_offsets ([B + 1] int32: rows row_offsets[b] .. row_offsets[b + 1] of flat_idx are
        sequence b's, in ascending order; the rows behind row_offsets[B] hold -1) the last layer can still be evaluated at those
        rows only.  cap given: the sync-free form -- index generation and label compaction stay on
        the device, exactly `cap` rows come back (those beyond the real count R are zero rows whose label is -1) together
        with the compact int32 labels.  Neither: R is read back from the device (one host sync).
        pack: the encoder runs on the padding-free layout; the dense [MASK] indices are mapped to its rows."""
        self._mask_flag = None
        self._row_offsets = None

        def positions(ids_first, raw_first):
            if cap is not None:
                # more [MASK] positions than cap = B x max_masked_per_row: the offsets stay inside the cap (the masked-query
                # kernels index rows by them) and the loss comes back NaN -- through the packed layout's flag when that one is
                # folded into the loss anyway, else through this call's own
                pk_flag = self._packed.ids_packed if (self._packed is not None and n_real_tokens is not None) else None
                counts, offsets, flat, mx = self._match_positions(ids_first, raw_first, cap, pk_flag)
                self._mask_flag = mx if pk_flag is None else None
                lab = ops.compact_labels(labels_padded, counts, offsets, cap, flat)     # also sets flat[R:] = -1
                self._row_offsets = offsets
                return flat, offsets, lab
            _, offsets, flat, _ = self._match_positions(ids_first, raw_first)
            self._row_offsets = offsets          # [B + 1]: rows offsets[b] .. offsets[b + 1] are sequence b's (predict_topk)
            R = int(offsets[-1].item())
            return flat[:R], offsets, None

        # The positions depend on the ids alone.  With them in hand BEFORE the encoder runs, its last layer is evaluated
        # for those rows only (ops.MQAttnBlockFn): nothing else of that layer's output is ever read on this path.
        # (in training with attention dropout only with ops.mq_attn_dropout: without it the full layer runs and its rows are gathered)
        given = flat_idx is not None and row_offsets is not None
        mq = (flat_idx is None or given) and ops.mq_last_layer and self.transformer.encoder.rows_route(None, bool(training))
        if mq and given:
            # the caller's rows and their per-sequence offsets (a next-item evaluation batch carries both): the same route; the rows
            # behind row_offsets[B] belong to no sequence and stay zeros
            dev = self.transformer.position_table.device
            off = torch.as_tensor(row_offsets).to(device=dev, dtype=torch.int32)
            self._row_offsets = off

            def named(ids_first, raw_first):
                fi = flat_idx(ids_first) if callable(flat_idx) else flat_idx
                return torch.as_tensor(fi).to(device=dev, dtype=torch.int32), off, None
            rows, _, _, _, _ = self._encode(inputs, training, pack, n_real_tokens, rows_of=named)
            return rows, None
        if mq:
            rows, _, _, _, _ = self._encode(inputs, training, pack, n_real_tokens, rows_of=positions)
            return rows, self._rows_extra
        enc, ids_first, raw_first, _, _ = self._encode(inputs, training, pack, n_real_tokens)
        d = enc.shape[-1]
        lab = None
        if flat_idx is None:
            flat_idx, _, lab = positions(ids_first, raw_first)
        elif callable(flat_idx):
            flat_idx = torch.as_tensor(flat_idx(ids_first)).to(device=enc.device, dtype=torch.int32)
        if self._packed is not None:
            flat_idx = ops.remap_index(flat_idx.contiguous(), self._packed.packed_of)
        rows = ops.GatherRowsFn.apply(enc.reshape(-1, d), flat_idx, flat_idx.shape[0])
        return rows, lab

    def _loss_rows(self, inputs, labels, training, flat_idx, max_masked_per_row, packed, n_real_tokens):
        """what the training losses share -> (rows [R, d] at the [MASK] positions, compact int32 labels [R], poison): the forms of
        cloze_loss's docstring.  poison: None, or the int32 device flag whose negative value must turn the loss into NaN."""
        pack = self._use_packed(inputs, packed, n_real_tokens)
        lab = torch.as_tensor(labels, device=self.transformer.position_table.device)
        if max_masked_per_row is not None and flat_idx is None:
            if lab.dim() != 2:
                raise ValueError('the sync-free form needs the padded (B, M) labels')
            rows, lab = self._masked_rows(inputs, training, None, cap=int(lab.shape[0]) * int(max_masked_per_row),
                                          labels_padded=lab, pack=pack, n_real_tokens=n_real_tokens)
        else:
            rows, _ = self._masked_rows(inputs, training, flat_idx, pack=pack, n_real_tokens=n_real_tokens)
            if lab.dim() == 2:
                lab = lab[lab != -1.0]
            lab = lab.to(torch.int32).contiguous()
            if lab.shape[0] != rows.shape[0]:
                raise ValueError('%d labels for %d masked positions' % (lab.shape[0], rows.shape[0]))
        # a wrong n_real_tokens would silently drop or invent tokens, more [MASK] positions than B x max_masked_per_row
        # would drop rows: the device-side counts disagree -> NaN loss (no read-back)
        poison = self._packed.ids_packed if (self._packed is not None and n_real_tokens is not None) else self._mask_flag
        return rows, lab, poison

    def cloze_loss(self, inputs, labels, training=True, flat_idx=None, variant='tf', unit_grad=False, max_masked_per_row=None,
                   packed=None, n_real_tokens=None):
        """Masked-item training loss == ClozeMaskedLoss(sparse_categorical_crossentropy)(labels, self(inputs)).
        labels: (B, M) float32 padded with -1 (reference format) or compact (R,) int ids in row-major mask order.
        flat_idx (R,) int32 skips the device-side index generation.  max_masked_per_row=M (the pipeline's
        MAX_MASKED_ITEMS, cloze_constants.py:1) selects the sync-free form: [MASK] positions and the labels of the padded
        (B, Mlab) tensor are compacted on the device, the head runs on B*M rows (the unused ones are ignored rows), and no
        value is read back to the host.
        n_real_tokens (host int: non-pad positions of the chained batch, which the input pipeline knows when it pads) /
        packed: run the encoder on the padding-free layout (bf16 throughput path; same loss and gradients, the pad
        positions' work is not done)."""
        rows, lab, poison = self._loss_rows(inputs, labels, training, flat_idx, max_masked_per_row, packed, n_real_tokens)
        code = CE_TF if variant == 'tf' else CE_PLAIN
        if hasattr(self.head, 'cloze_ce'):
            if poison is not None and getattr(self.head, 'accepts_poison', False):
                loss = self.head.cloze_ce(rows, lab, code, unit_grad, poison=poison)      # folded into the loss kernel
                poison = None
            else:
                loss = self.head.cloze_ce(rows, lab, code, unit_grad)
        else:
            loss = ops.FusedSoftmaxCEFn.apply(self.head.logits(rows), lab, self.head.output_vocab_size, code, unit_grad, poison)
            poison = None
        if poison is not None:
            loss = loss + torch.where(poison[0] < 0, float('nan'), 0.0).to(loss.dtype)
        return loss

    CANDIDATE_LOSSES = ('bce', 'softmax', 'bpr', 'gbce')

    @staticmethod
    def gbce_beta(num_negatives, num_items, t):
        """gSASRec's exponent of the positive probability (Petrov & Macdonald 2023), here the weight of the target's BCE term:
        beta = alpha * (t * (1 - 1 / alpha) + 1 / alpha) with the sampling rate alpha = N / (V - 1); t = 0: 1 (BCE), t = 1: alpha."""
        alpha = float(num_negatives) / float(num_items - 1)
        return alpha * (float(t) * (1.0 - 1.0 / alpha) + 1.0 / alpha)

    def _candidate_loss_options(self, who, loss, gbce_t, logq, correct_target, extra=()):
        """the host checks of the loss keywords candidate_loss and next_item_loss share (before any device work)"""
        names = tuple(extra) + self.CANDIDATE_LOSSES
        if loss not in names:
            raise B4CError('%s: loss %r (%s or %r)' % (who, loss, ', '.join(repr(n) for n in names[:-1]), names[-1]))
        try:
            ok = 0.0 <= float(gbce_t) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise B4CError('%s: gbce_t = %r (the calibration parameter t of gBCE, in [0, 1])' % (who, gbce_t))
        if logq is None and correct_target:
            raise B4CError('%s: correct_target=True needs logq (there is no correction to apply to the target)' % who)
        if logq is not None and (not isinstance(logq, torch.Tensor) or logq.dtype != torch.float32 or logq.dim() != 1):
            raise B4CError('%s: logq must be a device fp32 [V] tensor (cloze.log_expected_count)' % who)

    def candidate_loss(self, inputs, labels, candidates=None, num_negatives=None, loss='bce', exclude=None, item_cdf=None, seed=None,
                       row_base=0, training=True, flat_idx=None, unit_grad=False, max_masked_per_row=None, packed=None,
                       n_real_tokens=None, gbce_t=0.75, logq=None, correct_target=False):
        """Sampled-negative training loss: each masked row against its own list of items, the label first -- loss='bce' (SASRec:
        softplus(-s_label) + the sum of softplus(s_negative)), 'softmax' (the list-wise softmax over the label and the negatives,
        the loss of the sampled-negative HitRate / NDCG protocol), 'bpr' (the sum over the negatives of softplus(s_negative -
        s_label)) or 'gbce' (gSASRec: 'bce' with the label's term times beta = gbce_beta(N, V, gbce_t), N the negatives per list,
        which undoes the over-confidence of BCE with few negatives; gbce_t in [0, 1], 0 is 'bce') -- mean over the rows with a valid
        label.  logq (device fp32 [V], cloze.log_expected_count of the counts the lists are drawn by): the sampled-softmax logQ
        correction -- every negative is scored s - logq[item]; the label too only with correct_target=True (it stands in its list
        with probability 1).  The head's projection
        is read and receives gradient at the listed rows only (head.candidate_loss; ClozeMaskedItemPrediction, SampledSoftmaxHead).
        inputs, labels, training, flat_idx, max_masked_per_row, packed, n_real_tokens: as in cloze_loss, the sync-free form and the
        NaN loss on a contradicted token count included.  Exactly one of
          candidates:    integer lists (label space; < 0 or >= V: absent), (R, C) one per masked row or (B, C) one per sequence,
                         C <= 1024, whose column 0 is the row's label: a row where it is not turns the loss into NaN (checked on
                         the device, no read-back);
          num_negatives: the lists are drawn here (ops.sample_candidates: never the label, never an item of `exclude`, uniform or
                         by item_cdf), a pure function of (seed, row_base + row); seed None: the next of the model's dropout seeds.
        exclude: (R, E) or (B, E) as in predict_topk -- e.g. the user's own items."""
        if (candidates is None) == (num_negatives is None):
            raise B4CError('candidate_loss: give exactly one of candidates and num_negatives')
        self._candidate_loss_options('candidate_loss', loss, gbce_t, logq, correct_target)
        if not hasattr(self.head, 'candidate_loss'):
            raise B4CError('candidate_loss: the head %s has no vocabulary projection to score items with' % type(self.head).__name__)
        rows, lab, poison = self._loss_rows(inputs, labels, training, flat_idx, max_masked_per_row, packed, n_real_tokens)
        V = self.head.output_vocab_size
        bad = None
        if candidates is not None:
            if exclude is not None or item_cdf is not None:
                raise B4CError('candidate_loss: exclude / item_cdf shape the lists drawn here; leave such items out of `candidates`')
            cand = self._row_candidates(candidates, rows.shape[0], rows.device, 'candidate_loss')
            lab_ok = (lab >= 0) & (lab < V)
            bad = (lab_ok & (cand[:, 0] != lab)).any()
            cand = torch.cat([torch.where(lab_ok, lab, torch.full_like(lab, -1))[:, None], cand[:, 1:]], 1)
        else:
            ex = self._row_exclusions(exclude, rows.shape[0], rows.device, lab) if exclude is not None else None
            from .transformer import dropout_seeds
            cand, _ = ops.sample_candidates(lab, V, num_negatives, dropout_seeds.next() if seed is None else seed, row_base, ex, item_cdf)
        kind, kw = loss, {}
        if loss == 'gbce':
            N = int(cand.shape[1]) - 1
            if N < 1 or V < 2:
                raise B4CError("candidate_loss: 'gbce' needs at least one negative per list and two items (N = %d, V = %d)" % (N, V))
            kind, beta = 'bce', self.gbce_beta(N, V, gbce_t)
            if beta != 1.0:
                kw['beta'] = beta
        if logq is not None:
            if logq.numel() != V:
                raise B4CError('candidate_loss: logq has %d entries for V = %d items' % (logq.numel(), V))
            kw.update(corr=logq, correct_target=bool(correct_target))
        out = self.head.candidate_loss(rows, cand, kind, unit_grad, **kw)
        if poison is not None:
            out = out + torch.where(poison[0] < 0, float('nan'), 0.0).to(out.dtype)
        if bad is not None:
            out = out + torch.where(bad, float('nan'), 0.0).to(out.dtype)
        return out

    def next_item_loss(self, batch, loss='full', variant='tf', unit_grad=False, training=True, gbce_t=0.75, logq=None,
                       correct_target=False):
        """Next-item training loss of a device-built batch (cloze_batches.DeviceCloze.next_item_batches): every real position of
        the unmasked rows predicts the item after it.  loss 'full': cloze_loss over the whole vocabulary (variant as there);
        'bce' / 'softmax' / 'bpr' / 'gbce': candidate_loss over the batch's own lists (built with num_negatives > 0), with its
        gbce_t, logq and correct_target.  A thin entry: the batch's
        flat_idx, labels, candidates and n_real_tokens go to those two methods, whose NaN conventions carry over; compact rows
        past the batch's targets (rows=) are ignored rows.  A model with side features -- every chain naming ONE input, so that each
        is laid out [CLS] [SEP] values .. [SEP] as the batch's flat_idx expects -- takes them from batch['features'] by name
        (DeviceCloze(features=...)); the first chain's input is the items.  Names the model does not use are ignored."""
        self._candidate_loss_options('next_item_loss', loss, gbce_t, logq, correct_target, extra=('full',))
        inputs = self._next_item_inputs(batch)
        if loss == 'full':
            return self.cloze_loss(inputs, batch['labels'], training=training, flat_idx=batch['flat_idx'], variant=variant,
                                   unit_grad=unit_grad, n_real_tokens=batch['n_real_tokens'])
        if batch.get('candidates') is None:
            raise B4CError('next_item_loss: loss %r needs the batch\'s candidate lists; build it with num_negatives > 0' % (loss,))
        return self.candidate_loss(inputs, batch['labels'], candidates=batch['candidates'], loss=loss, training=training,
                                   flat_idx=batch['flat_idx'], unit_grad=unit_grad, n_real_tokens=batch['n_real_tokens'], gbce_t=gbce_t,
                                   logq=logq, correct_target=correct_target)

    CONTRASTIVE_SIMILARITIES = ('dot', 'cos')

    def _sequence_rows(self, inputs, flat_idx, training, packed, n_real_tokens):
        """one encoder row per sequence -> (B, d): at flat_idx ((B,) int32, b * S + s), or by default at each sequence's last item --
        the last non-pad position in front of the chain's closing [SEP], index (non-pad count) - 2 of a right-padded row [CLS] [SEP]
        items .. [SEP], from the counts the device already has (the packed layout's, else one b4c_nonpad_positions launch)."""
        pack = self._use_packed(inputs, packed, n_real_tokens)

        def last_items(ids_first):
            B, S = ids_first.shape
            if self._packed is not None:
                counts = self._packed.cu[1:] - self._packed.cu[:-1]
            else:
                counts = ops.nonpad_positions(ids_first.contiguous(), B * S)[0]
            return (torch.arange(B, dtype=torch.int32, device=ids_first.device) * S + (counts.to(torch.int32) - 2).clamp(min=0))

        if flat_idx is None:
            fi = last_items
        else:
            fi = torch.as_tensor(flat_idx, device=self.transformer.position_table.device).to(torch.int32).reshape(-1)
        first_in = self.sequential_input_config[list(self.sequential_input_config.keys())[0]][0]
        x = inputs[first_in]
        B = int(x.shape[0]) if isinstance(x, torch.Tensor) else int(np.asarray(x, dtype=object).shape[0])
        if flat_idx is not None and fi.shape[0] != B:
            raise B4CError('contrastive_loss: flat_idx names %d rows for %d sequences (one position per sequence)' % (fi.shape[0], B))
        off = torch.arange(B + 1, dtype=torch.int32, device=self.transformer.position_table.device)
        rows, _ = self._masked_rows(inputs, training, fi, pack=pack, n_real_tokens=n_real_tokens, row_offsets=off)
        return rows

    def contrastive_loss(self, inputs, inputs_b=None, flat_idx=None, temperature=1.0, similarity='dot', same_target=None, training=True,
                         packed=None, n_real_tokens=None, n_real_tokens_b=None):
        """In-batch contrastive loss between two views of the batch's B sequences (InfoNCE / NT-Xent: the auxiliary loss of CL4SRec
        and DuoRec), a scalar to add to any of the training losses:
            loss = model.next_item_loss(batch) + lam * model.contrastive_loss(inputs, ...)
        A sequence's representation is its encoder row at one position: flat_idx ((B,) int32, b * S + s, the same for both views), by
        default the position of its last item (found on the device, no host loop).  A model on the masked-query route evaluates its
        last layer at those B rows only.
        Views.  inputs_b given: the second view, B sequences the caller augmented (CL4SRec: crop / mask / reorder; DuoRec: the row
        of another sequence in front of the same target) -- cloze_batches.DeviceCloze.views builds them on the device; its
        view['n_real_tokens'] as n_real_tokens_b lets the second view take the padding-free layout too (None: the dense one, unless
        packed=True).  inputs_b None: the
        same inputs are encoded twice under two successive draws of the dropout seeds (DuoRec's unsupervised view, SimCSE); that needs
        training=True and dropout_rate > 0 -- otherwise the two views are identical and the loss a constant: B4CError.
        Loss.  z = cat(rows_a, rows_b) (2B rows), the positive of row i is the other view of its sequence, the negatives are every
        other row of the 2B; same_target ((B,) integer, negative: none; DuoRec): two sequences with the same target item are not
        each other's negatives.  s = z_i . z_j / temperature ('dot') or the rows' cosine / temperature ('cos'); mean over the 2B rows
        of logsumexp over the keys - s at the positive.  One fused kernel pair (ops.InfoNCEFn, include/b4c.h): the [2B, 2B]
        scores never reach memory; d_model must be a multiple of 8, at most 128.
        Cost: two more encoder passes on top of the main loss's (one per view).  Under data parallelism the negatives are the rank's
        own batch: there is no all-gather.  No reference oracle (the reference trains with the Cloze loss alone); the float64
        restatement is tests/nce_ref.py."""
        if similarity not in self.CONTRASTIVE_SIMILARITIES:
            raise B4CError("contrastive_loss: similarity %r ('dot' or 'cos')" % (similarity,))
        if inputs_b is None and not (training and float(self.dropout_rate) > 0.0):
            raise B4CError('contrastive_loss: inputs_b=None takes its two views from two dropout realisations of the same inputs; that '
                           'needs training=True and dropout_rate > 0 (here training=%r, dropout_rate=%g): the views would be identical '
                           'and the loss constant.  Pass an augmented second view as inputs_b.' % (bool(training), float(self.dropout_rate)))
        rows_a = self._sequence_rows(inputs, flat_idx, training, packed, n_real_tokens)
        rows_b = self._sequence_rows(inputs if inputs_b is None else inputs_b, flat_idx, training, packed,
                                     n_real_tokens if inputs_b is None else n_real_tokens_b)
        B = rows_a.shape[0]
        if rows_b.shape[0] != B:
            raise B4CError('contrastive_loss: the two views hold %d and %d sequences' % (B, rows_b.shape[0]))
        dev = rows_a.device
        z = torch.cat([rows_a, rows_b], 0)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        pos = torch.cat([idx + B, idx])
        group = None
        if same_target is not None:
            g = torch.as_tensor(same_target, device=dev).reshape(-1)
            if g.shape[0] != B or g.is_floating_point():
                raise B4CError('contrastive_loss: same_target must be a (B,) = (%d,) integer tensor (negative: none)' % B)
            g = g.to(torch.int32)
            group = torch.cat([g, g])
        return ops.InfoNCEFn.apply(z, pos, group, float(temperature), similarity)

    def _next_item_inputs(self, batch):
        """the model's inputs of a next-item batch (no device work).  Every chain names one input: the layout [CLS] [SEP] values ..
        [SEP] the batch's flat_idx is built for; the first chain's is the items, the others come from batch['features'] by name."""
        chains = list(self.sequential_input_config.values())
        if not chains or any(len(chain) != 1 for chain in chains):
            raise B4CError('next_item_loss: every chain of the model must name exactly one input (the batch\'s positions are those of '
                           '[CLS] [SEP] items .. [SEP]), got %s' % (chains,))
        names = [chain[0] for chain in chains]
        inputs = {names[0]: batch['items']}
        have = batch.get('features') or {}
        for name in names[1:]:
            if name not in have:
                raise B4CError('next_item_loss: the model takes the feature %r, which the batch does not carry (it has %s); build the '
                               'batches with DeviceCloze(features={%r: Feature(...)})' % (name, sorted(have) or 'none', name))
            inputs[name] = have[name]
        return inputs

    @torch.no_grad()
    def predict_topk(self, inputs, k, labels=None, flat_idx=None, packed=None, n_real_tokens=None, exclude=None, candidates=None,
                     row_offsets=None):
        """Top-k item ids (label space) at every masked position, ranked over all V items: the fp32 path ranks the fp32
        probabilities as the reference's metrics do (utils.py:176, 245), the bf16 path the fp32 logits (head.SoftMaxHead.topk);
        returns (topk_idx (R,k) int32, hit (R,), ndcg (R,)) -- the latter two when labels are given.
        exclude: items (label space) left out of the ranking -- an integer tensor padded with negative ids, or a host list of
        lists: (R, E) one list per masked row in row-major order, or (B, E) one per sequence, for each of its [MASK] rows (a
        first dimension equal to R is read per row).  An excluded item is never returned and never ranks before the label;
        the label itself is never excluded; fewer than k items left: ids -1.
        candidates: the ranking is limited to a list of items per row (label space; < 0 or >= V: absent) -- an integer tensor
        (R, C) one list per masked row, or (B, C) one per sequence, C <= 1024 (cloze.sample_candidates for the sampled-negative
        protocol); the fp32 logits of the listed items are ranked, the label counts only where it is listed, and hit / ndcg
        come from the label's rank among the listed items.  Not together with exclude.
        row_offsets (with flat_idx; a next-item batch's b['row_offsets']): the [B + 1] int32 offsets of the compact rows per
        sequence.  With them the last encoder layer is evaluated at the given rows only where that route is open
        (ops.mq_last_layer, Encoder.rows_route: a bidirectional model, or a causal one with ops.mq_causal), and (B, ...) exclude /
        candidates lists are spread over the rows by them; without them, or with the route closed, the full last layer runs and
        its rows are gathered."""
        if candidates is not None and exclude is not None:
            raise B4CError('predict_topk: candidates and exclude together; leave excluded items out of the lists')
        rows, _ = self._masked_rows(inputs, False, flat_idx, pack=self._use_packed(inputs, packed, n_real_tokens),
                                    n_real_tokens=n_real_tokens, row_offsets=row_offsets)
        lab = None
        if labels is not None:
            lab = torch.as_tensor(labels, device=rows.device)
            if lab.dim() == 2:
                lab = lab[lab != -1.0]
            lab = lab.to(torch.int32).contiguous()
        ex = None
        if exclude is not None:
            ex = self._row_exclusions(exclude, rows.shape[0], rows.device, lab)
        if candidates is not None:
            cand = self._row_candidates(candidates, rows.shape[0], rows.device, 'predict_topk')
            if hasattr(self.head, 'score_candidates'):
                _, rank, idx = self.head.score_candidates(rows, cand, lab, k, want_scores=False)
            else:
                rank, idx = ops.candidate_rank_rows(self.head.logits(rows, out_fp32=True), self.head.output_vocab_size, cand, lab, k)
            hit, ndcg = ops.rank_metrics(rank, k) if rank is not None else (None, None)
        elif hasattr(self.head, 'topk'):           # logits-free where the head's kernels cover it (head.SoftMaxHead.topk)
            idx, hit, ndcg = self.head.topk(rows, k, lab, exclude=ex)
        else:
            scores = self.head.logits(rows, out_fp32=True)
            if rows.dtype == torch.float32:
                scores = ops.softmax_rows(scores, self.head.output_vocab_size)
            idx, hit, ndcg = ops.topk_rows(scores, self.head.output_vocab_size, k, lab, exclude=ex)
        if self._packed is not None and n_real_tokens is not None:
            # a caller-given token count that the device's own contradicts: ids -1, hit / ndcg NaN (no read-back)
            flag = self._packed.ids_packed
            ops.poison_rows(idx, flag)
            if hit is not None:
                ops.poison_rows(hit.view(-1, 1), flag)
                ops.poison_rows(ndcg.view(-1, 1), flag)
        return idx, hit, ndcg

    @torch.no_grad()
    def score_candidates(self, inputs, candidates, labels=None, flat_idx=None, packed=None, n_real_tokens=None, row_offsets=None):
        """fp32 logits (R, C) of each [MASK] row's own candidate list (label-space ids; an id < 0 or >= V is absent and scores
        NaN): the head's projection at the listed items only (head.SoftMaxHead.score_candidates, b4c_candidate_score).
        candidates: an integer tensor (R, C) one list per masked row in row-major order, or (B, C) one per sequence, C <= 1024.
        labels are not needed for the scores; they are accepted as predict_topk accepts them (and ignored).
        row_offsets: as in predict_topk."""
        rows, _ = self._masked_rows(inputs, False, flat_idx, pack=self._use_packed(inputs, packed, n_real_tokens),
                                    n_real_tokens=n_real_tokens, row_offsets=row_offsets)
        cand = self._row_candidates(candidates, rows.shape[0], rows.device, 'score_candidates')
        if hasattr(self.head, 'score_candidates'):
            scores, _, _ = self.head.score_candidates(rows, cand)
        else:
            raise B4CError('score_candidates: the head %s has no vocabulary projection to score items with' % type(self.head).__name__)
        if self._packed is not None and n_real_tokens is not None:
            ops.poison_rows(scores, self._packed.ids_packed)      # contradicted token count: NaN rows (no read-back)
        return scores

    def _row_candidates(self, candidates, R, device, who):
        """(R, C) or (B, C) integer candidate lists -> int32 (R, C) on the device, one list per masked row"""
        c = torch.as_tensor(candidates)
        if c.dim() != 2 or c.dtype.is_floating_point or c.dtype == torch.bool:
            raise B4CError('%s: candidates must be an integer (R, C) or (B, C) tensor, got %s %s' % (who, c.dtype, tuple(c.shape)))
        if c.dtype != torch.int32:          # ids outside the int32 range cannot be items: absent
            c = torch.where((c >= 0) & (c < self.head.output_vocab_size), c, torch.full_like(c, -1)).to(torch.int32)
        c = c.to(device)
        if c.shape[0] != R:
            offsets = self._row_offsets
            if offsets is None or c.shape[0] != offsets.shape[0] - 1:
                raise B4CError('%s: candidates have %d lists for %d masked rows%s' % (
                    who, c.shape[0], R, '' if offsets is None else ' of %d sequences' % (offsets.shape[0] - 1)))
            c = c[self._sequence_of_rows(R, device)]
        return c.contiguous()

    def _sequence_of_rows(self, R, device):
        """the sequence of each of the R masked rows (self._row_offsets).  The sync-free form runs on more rows than there are
        [MASK] positions: the rows past the last one are ignored rows and are given the last sequence's list"""
        offsets = self._row_offsets
        seq = torch.searchsorted(offsets[1:].long(), torch.arange(R, device=device), right=True)
        return seq.clamp_(max=offsets.shape[0] - 2)

    def _row_exclusions(self, exclude, R, device, lab):
        """predict_topk's `exclude` -> the canonical (R, E) lists of ops.exclusions, one per masked row"""
        if not isinstance(exclude, torch.Tensor):
            exclude = ops.exclusions(exclude, 1 << 30)         # host lists -> one int32 tensor, -1 padded (ids kept as given)
        if exclude.dim() != 2:
            raise B4CError('predict_topk: exclude must be (R, E) or (B, E), got shape %s' % (tuple(exclude.shape),))
        exclude = exclude.to(device)
        if exclude.shape[0] != R:
            offsets = self._row_offsets
            if offsets is None or exclude.shape[0] != offsets.shape[0] - 1:
                raise B4CError('predict_topk: exclude has %d lists for %d masked rows%s' % (
                    exclude.shape[0], R, '' if offsets is None else ' of %d sequences' % (offsets.shape[0] - 1)))
            exclude = exclude[self._sequence_of_rows(R, device)]
        return ops.exclusions(exclude, self.head.output_vocab_size, lab)

    def get_serving_signature(self):
        names = []
        for chain in self.sequential_input_config.values():
            names.extend(chain)
        return {n: ('string', [None, None]) for n in names}
