"""Mirror of ``bm/models/convrnn.py``: ``LSTM``, ``Attention`` and ``ConvRNN`` (the reference's ``model=convrnn`` and
``model=decoder_convrnn``), decode direction: strided ConvSequence encoders -> LSTM stack -> optional local attention
-> transposed ConvSequence decoder -> optional head.

Same constructor keywords and defaults, module names and construction order as the reference, because ``state_dict``
keys, their order and the order of the random draws are the interoperability contract (a reference checkpoint loads;
tests/golden/make_convrnn_golden.py asserts bit-equal same-seed parameters).  Every ``forward`` is written over the
HIP ops: the encoders / decoder are ``ConvSequence`` (csrc/conv_strided.hip), the recurrence is ``BF.LSTMFn``
(csrc/lstm.hip), every 1x1 conv is ``BF.Conv1dFn``.  CPU tensors raise: there is no fallback.
"""
import math
import typing as tp

import torch
from torch import nn
from torch.nn import functional as F

from .. import functional as BF
from .. import hip_ops as H
from .common import ConvSequence, ScaledEmbedding, SubjectLayers, _Activation


class LSTM(nn.Module):
    """bm/models/convrnn.py:18-38: an LSTM stack whose output has ``hidden_size`` channels whether it is bidirectional
    or not (a ``2H -> H`` linear map follows the bidirectional one).

    ``self.lstm`` is an ``nn.LSTM`` held purely as the parameter container (keys, shapes, initialisation); its forward
    is never called.  The recurrence is ``BF.LSTMFn``; the linear map runs as a 1x1 HIP conv.  Works on [B, C, T]
    (the reference permutes to [T, B, C] around it): returns (y [B, H, T], (h_n, c_n))."""

    def __init__(self, input_size, hidden_size, num_layers, dropout, bidirectional):
        super().__init__()
        self.lstm = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                            bidirectional=bidirectional)
        self.linear = None
        if bidirectional:
            self.linear = nn.Linear(2 * hidden_size, hidden_size)

    def forward(self, x):
        rnn = self.lstm
        y, h_n, c_n = BF.LSTMFn.apply(x, rnn.hidden_size, rnn.num_layers, rnn.bidirectional, float(rnn.dropout),
                                      self.training, *[getattr(rnn, name) for name in rnn._flat_weights_names])
        if self.linear is not None:
            y = BF.Conv1dFn.apply(y, self.linear.weight[:, :, None], self.linear.bias, 1, H.ACT_NONE, 0., False)
        return y, (h_n, c_n)


class Attention(nn.Module):
    """bm/models/convrnn.py:41-88: multi-head attention over the time axis with learnt relative-position embeddings;
    offsets beyond ``radius`` share the table's outermost rows.

    Off the hot path (``attention`` is 0 in every configuration of the reference), so it is correct, not tuned: the
    four 1x1 convs (content, query, key, fc) are ``BF.Conv1dFn``; the scores, the softmax, the embedding terms and the
    BatchNorm are GPU torch ops restated from the formulas, materialising the [T, T, C / heads] embedding table:

        score[b,h,t,s] = <q[b,h,:,t], k[b,h,:,s]> + 0.3 <q[b,h,:,t], E[clamp(t - s)]>
        w = softmax_s(score);   out[b,h,:,t] = sum_s w[b,h,t,s] (content[b,h,:,s] + 0.3 E[clamp(t - s)])
        result = relu(bn(fc(out))) * scale

    What the reference computes, as the fixture pins it (``long_attention``, T' = 62): it clamps the offsets IN PLACE
    before it compares them with the radius, so its "outside the radius" mask never removes a score -- every step
    attends to every other step, distant ones through the clamped embedding row.  Restated as such: no mask."""

    def __init__(self, channels: int, radius: int = 50, heads: int = 4):
        super().__init__()
        assert channels % heads == 0
        self.content = nn.Conv1d(channels, channels, 1)
        self.query = nn.Conv1d(channels, channels, 1)
        self.key = nn.Conv1d(channels, channels, 1)
        self.embedding = nn.Embedding(radius * 2 + 1, channels // heads)
        # the reference smooths the table: running sum over positions, divided by sqrt(position + 1)
        table = self.embedding.weight.data
        table[:] = table.cumsum(0) / torch.arange(1, len(table) + 1).float().view(-1, 1).sqrt()
        self.heads = heads
        self.radius = radius
        self.bn = nn.BatchNorm1d(channels)
        self.fc = nn.Conv1d(channels, channels, 1)
        self.scale = nn.Parameter(torch.full([channels], 0.1))

    @staticmethod
    def _conv(mod, x):
        return BF.Conv1dFn.apply(x, mod.weight, mod.bias, 1, H.ACT_NONE, 0., False)

    def forward(self, x):
        B, C, T = x.shape
        heads = self.heads
        content = self._conv(self.content, x).view(B, heads, C // heads, T)
        query = self._conv(self.query, x).view(B, heads, C // heads, T)
        key = self._conv(self.key, x).view(B, heads, C // heads, T)
        steps = torch.arange(T, device=x.device)
        delta = steps[:, None] - steps[None, :]                           # [t, s] = t - s
        emb = self.embedding.weight[(delta.clamp(-self.radius, self.radius) + self.radius)]      # [T, T, C / heads]
        scores = torch.einsum("bhct,bhcs->bhts", query, key) + 0.3 * torch.einsum("bhct,tsc->bhts", query, emb)
        weights = torch.softmax(scores, dim=-1)
        out = torch.einsum("bhts,bhcs->bhct", weights, content) + 0.3 * torch.einsum("bhts,tsc->bhct", weights, emb)
        out = self._conv(self.fc, out.reshape(B, C, T).contiguous())
        return F.relu(self.bn(out)) * self.scale.view(1, -1, 1)


class ConvRNN(nn.Module):
    """bm/models/convrnn.py:91-274, same keywords and defaults.  ``forward(inputs, batch)`` is what ``Solver`` calls:
    ``inputs`` maps input names to [B, C, T] GPU tensors, ``batch.subject_index`` holds the subjects.

    Not built: the ``encode`` task (MEG as the target), which lives outside the model in the reference."""

    def __init__(self,
                 # Channels
                 in_channels: tp.Dict[str, int],
                 out_channels: int,
                 hidden: tp.Dict[str, int],
                 # Overall structure
                 depth: int = 2,
                 linear_out: bool = False,
                 complex_out: bool = False,
                 concatenate: bool = False,
                 # Conv structure
                 kernel_size: int = 4,
                 stride: int = 2,
                 growth: float = 1.,
                 # LSTM
                 lstm: int = 2,
                 flip_lstm: bool = False,
                 bidirectional_lstm: bool = False,
                 # Attention
                 attention: int = 0,
                 heads: int = 4,
                 # Dropout, BN, activations
                 conv_dropout: float = 0.0,
                 lstm_dropout: float = 0.0,
                 dropout_input: float = 0.0,
                 batch_norm: bool = False,
                 relu_leakiness: float = 0.0,
                 # Subject embeddings
                 n_subjects: int = 200,
                 subject_dim: int = 64,
                 embedding_location: tp.List[str] = ["lstm"],      # "lstm", "input" or both
                 embedding_scale: float = 1.0,
                 subject_layers: bool = False,
                 subject_layers_dim: str = "input",                # or "hidden"
                 ):
        super().__init__()
        if set(in_channels.keys()) != set(hidden.keys()):
            raise ValueError("Channels and hidden keys must match "
                             f"({set(in_channels.keys())} and {set(hidden.keys())})")
        in_channels = dict(in_channels)        # (the reference edits its caller's dict; the widths below are the same)
        hidden = dict(hidden)
        self._concatenate = concatenate
        self.depth = depth
        self.kernel_size = kernel_size
        self.stride = stride
        self.embedding_location = embedding_location

        self.subject_layers = None
        if subject_layers:
            assert "meg" in in_channels
            width = {"hidden": hidden["meg"], "input": in_channels["meg"]}[subject_layers_dim]
            self.subject_layers = SubjectLayers(in_channels["meg"], width, n_subjects)
            in_channels["meg"] = width
        self.subject_embedding = None
        if subject_dim:
            self.subject_embedding = ScaledEmbedding(n_subjects, subject_dim, embedding_scale)
            if "input" in embedding_location:
                in_channels["meg"] += subject_dim
        if concatenate:
            in_channels = {"concat": sum(in_channels.values())}
            hidden = {"concat": sum(hidden.values())}

        # channel widths of every encoder: its input, then hidden * growth^k
        widths = {name: [cin] + [int(round(hidden[name] * growth ** k)) for k in range(depth)]
                  for name, cin in in_channels.items()}
        lstm_hidden = sum(w[-1] for w in widths.values())
        lstm_input = lstm_hidden + (subject_dim if "lstm" in embedding_location else 0)

        conv_kw: tp.Dict[str, tp.Any] = dict(kernel=kernel_size, stride=stride, leakiness=relu_leakiness,
                                             dropout=conv_dropout, dropout_input=dropout_input, batch_norm=batch_norm)
        self.encoders = nn.ModuleDict({name: ConvSequence(w, **conv_kw) for name, w in widths.items()})

        self.lstm = None
        self.linear = None
        if lstm:
            self.lstm = LSTM(input_size=lstm_input, hidden_size=lstm_hidden, dropout=lstm_dropout, num_layers=lstm,
                             bidirectional=bidirectional_lstm)
            self._flip_lstm = flip_lstm

        self.attentions = nn.ModuleList(Attention(lstm_hidden, heads=heads) for _ in range(attention))

        decoder_widths = [int(round(lstm_hidden / growth ** k)) for k in range(depth + 1)]
        self.final = None
        if linear_out:
            assert not complex_out
            self.final = nn.Conv1d(decoder_widths[-1], out_channels, 1)
        elif complex_out:
            self.final = nn.Sequential(nn.Conv1d(decoder_widths[-1], 2 * decoder_widths[-1], 1), _Activation("relu"),
                                       nn.Conv1d(2 * decoder_widths[-1], out_channels, 1))
        else:
            conv_kw["activation_on_last"] = False
            decoder_widths[-1] = out_channels
            assert depth > 0, "if no linear out, depth must be > 0"
        self.decoder = ConvSequence(decoder_widths, decode=True, **conv_kw)

    def valid_length(self, length):
        """The smallest length >= ``length`` (for the reference's kernel 4 / stride 2) that the encoder -> decoder
        chain maps onto itself: ``depth`` times ceil(L / stride) + 1 going down, ``depth`` times (L - 1) * stride
        going up (bm/models/convrnn.py:209-223)."""
        for _ in range(self.depth):
            length = max(math.ceil(length / self.stride) + 1, 1)
        for _ in range(self.depth):
            length = (length - 1) * self.stride
        return int(length)

    def pad(self, x):
        return F.pad(x, (0, self.valid_length(x.size(-1)) - x.size(-1)))

    def forward(self, inputs, batch):
        subjects = batch.subject_index
        first = next(iter(inputs.values()))
        length = first.shape[-1]
        for name, value in inputs.items():
            if not value.is_cuda:
                raise RuntimeError("brainmagick_amd.ConvRNN runs on the MI355X HIP path only; got a "
                                   f"{value.device} tensor for {name!r} (there is no CPU fallback)")
            if value.dtype != torch.float32:
                raise TypeError(f"ConvRNN expects fp32 inputs like the reference, got {value.dtype} for {name!r}")

        if self.subject_layers is not None:
            inputs["meg"] = self.subject_layers(inputs["meg"].contiguous(), subjects)
        emb = None
        if self.subject_embedding is not None:
            emb = self.subject_embedding(subjects)[:, :, None]
            if "input" in self.embedding_location:
                inputs["meg"] = torch.cat([inputs["meg"], emb.expand(-1, -1, length)], dim=1)
        if self._concatenate:
            inputs = {"concat": torch.cat([value for _, value in sorted(inputs.items())], dim=1)}

        # the reference pads every input to its valid length, then once more on the way into the encoder
        encoded = {name: self.encoders[name](self.pad(self.pad(value)).contiguous()) for name, value in inputs.items()}
        parts = [value for _, value in sorted(encoded.items())]
        if emb is not None and "lstm" in self.embedding_location:
            parts.append(emb.expand(-1, -1, parts[0].shape[-1]))
        x = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]

        if self.lstm is not None:
            if self._flip_lstm:
                x = x.flip([2])
            x, _ = self.lstm(x)
            if self._flip_lstm:
                x = x.flip([2])
        for attention in self.attentions:
            x = x + attention(x.contiguous())
        x = self.decoder(x.contiguous())
        if isinstance(self.final, nn.Conv1d):
            x = BF.Conv1dFn.apply(x, self.final.weight, self.final.bias, 1, H.ACT_NONE, 0., False)
        elif self.final is not None:
            first_conv, act, last_conv = self.final
            x = BF.Conv1dFn.apply(x, first_conv.weight, first_conv.bias, 1, act.code, act.leak, False)
            x = BF.Conv1dFn.apply(x, last_conv.weight, last_conv.bias, 1, H.ACT_NONE, 0., False)
        return x[:, :, :length]
