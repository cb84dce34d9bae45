"""Mirror of the reference's ``src/models/LSTM.py``: ``LSTMRegressor``, a stacked LSTM over per-step expert features whose
last step feeds ``Linear(hidden_size, 15)``, trained with ``BCELoss`` on the sigmoid of the logits (the ``model: "lstm"``
branch of src/main.py:39-42).

Kept: the constructor signature and attribute names (``lstm``, ``linear``, ``criterion``, ``running_logits``,
``running_labels``, ``learning_rate`` ...), the state-dict keys of ``nn.LSTM`` + ``nn.Linear`` (a reference checkpoint
loads unchanged) and nn.LSTM's initialisation order, so one seed gives the reference's initial weights.

The recurrence runs on the HIP chain kernels (``functional.lstm_layer``), the sigmoid -> BCELoss criterion on one fused
kernel pair (``functional.sigmoid_bce``).  ``compute_dtype`` (attribute, default bf16) sets the activation dtype:
bf16 stores h, G and dG in bf16 with fp32 accumulation, gates and cell state; fp32 is exact fp32 arithmetic.

Deliberate deviations ("The LSTM baseline"):
  - ``configure_optimizers`` returns the HIP ``AdamW(weight_decay=0)``: the arithmetic of ``torch.optim.Adam``.
  - ``test_step`` does what the reference's intends (its ``result`` is never defined): the validation step's loss on a
    ``(x, y)`` batch, logged as ``test_loss``.
  - ``validation_step`` does not print the first label / prediction row.
  - A criterion other than ``nn.BCELoss()`` (mean, no weight) raises ``NotImplementedError``.
  - Training-mode dropout draws its masks from the Philox kernel: torch's generator stream is not reproduced.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .. import functional as F
from .. import ops
from .. import optim
from ..lightning_compat import LightningModule


class LSTM(nn.Module):
    """Parameters and forward of ``nn.LSTM(input_size, hidden_size, num_layers, batch_first=True, dropout)`` on the HIP
    chain.  ``forward(x)`` returns ``(output [B, T, H], h_last [B, H])``: the top layer's last hidden state instead of
    nn.LSTM's ``(h_n, c_n)`` tuple (the reference uses only ``output``)."""

    def __init__(self, input_size, hidden_size, num_layers=1, dropout=0.0, batch_first=True):
        super().__init__()
        if not batch_first:
            raise NotImplementedError("LSTM: only batch_first=True is implemented (LSTM.py:32-36)")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.dropout, self.batch_first = float(dropout), True
        for k in range(num_layers):                              # nn.LSTM's parameter order (its init draws in this order)
            fin = input_size if k == 0 else hidden_size
            self.register_parameter(f"weight_ih_l{k}", nn.Parameter(torch.empty(4 * hidden_size, fin)))
            self.register_parameter(f"weight_hh_l{k}", nn.Parameter(torch.empty(4 * hidden_size, hidden_size)))
            self.register_parameter(f"bias_ih_l{k}", nn.Parameter(torch.empty(4 * hidden_size)))
            self.register_parameter(f"bias_hh_l{k}", nn.Parameter(torch.empty(4 * hidden_size)))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def forward(self, x, compute_dtype=torch.bfloat16):
        h = F.cast(x, compute_dtype) if x.dtype != compute_dtype else x
        last = None
        for k in range(self.num_layers):
            if k > 0:
                h = F.dropout(h, self.dropout, self.training)
            h, last = F.lstm_layer(h, getattr(self, f"weight_ih_l{k}"), getattr(self, f"weight_hh_l{k}"),
                                   getattr(self, f"bias_ih_l{k}"), getattr(self, f"bias_hh_l{k}"))
        return h, last


class LSTMRegressor(LightningModule):
    def __init__(self,
                 n_features,
                 hidden_size,
                 seq_len,
                 batch_size,
                 num_layers,
                 dropout,
                 learning_rate,
                 criterion):
        super(LSTMRegressor, self).__init__()
        if not (isinstance(criterion, nn.BCELoss) and criterion.reduction == "mean" and criterion.weight is None):
            raise NotImplementedError(f"LSTMRegressor: only criterion=nn.BCELoss() (mean, no weight) has a HIP kernel, "
                                      f"got {criterion!r}")
        self.n_features = n_features
        self.hidden_size = hidden_size
        self.seq_len = seq_len
        self.batch_size = batch_size
        self.num_layers = num_layers
        self.dropout = dropout
        self.criterion = criterion
        self.running_logits = []
        self.running_labels = []
        self.learning_rate = learning_rate
        self.compute_dtype = torch.bfloat16
        self.lstm = LSTM(input_size=n_features, hidden_size=hidden_size, batch_first=True, num_layers=num_layers,
                         dropout=dropout)
        self.linear = nn.Linear(hidden_size, 15)

    def forward(self, x):
        """Logits [B, 15] (fp32) of ``linear(lstm(x)[0][:, -1])``."""
        _, last = self.lstm(x, self.compute_dtype)
        return F.linear(last, self.linear.weight, self.linear.bias, out_f32=True)

    def configure_optimizers(self):
        return optim.AdamW(self.parameters(), lr=self.learning_rate, weight_decay=0)

    @staticmethod
    def _batch(batch):
        x = torch.stack(batch["experts"]).squeeze(1)
        y = torch.cat(batch["label"]).squeeze(1).float()
        return x, y

    def loss(self, y_hat, y):
        """criterion(sigmoid(y_hat), y) as one kernel pair: nn.BCELoss (mean, log terms clamped at -100)."""
        return F.sigmoid_bce(y_hat, y)

    def training_step(self, batch, batch_idx):
        x, y = self._batch(batch)
        loss = self.loss(self(x), y)
        self.log('train_loss', loss)
        return loss

    def _eval_step(self, x, y, name):
        y_hat = self(x)
        with torch.no_grad():
            loss, prob = ops.sigmoid_bce_fwd(y_hat.detach().contiguous(), y.contiguous(), want_prob=True)
        loss = loss.view(())
        self.running_labels.append(y)
        self.running_logits.append(prob)
        self.log(name, loss)
        return loss

    def validation_step(self, batch, batch_idx):
        x, y = self._batch(batch)
        return self._eval_step(x, y, 'val_loss')

    def test_step(self, batch, batch_idx):
        x, y = batch
        return self._eval_step(x, y.float(), 'test_loss')
