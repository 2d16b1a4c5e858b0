"""Train and validation loops of the proposal generator with the reference's signatures, batch contract and TensorBoard tags
(epoch_loops/proposal_epoch_loops.py): batch = {'video_ids', 'feature_stacks', 'targets' (N, 4), 'duration_in_secs'} as
collate4proposal_generation builds it; model(feature_stacks, targets, masks) -> (predictions, loss, losses_A, losses_V).
The per-term losses stay device scalars while they are accumulated; the post-processing of the validation pass is one call
of ops.proposal_select per batch (proposal_utils.AnetPredictions)."""
import os

import torch

from ..model.masking import make_masks
from ..proposal_utils import AnetPredictions, add_dict_to_another_dict, calculate_f1, get_lr


def save_model(cfg, epoch, model, optimizer, scheduler, anet_metrics, best_metric):
    os.makedirs(cfg.log_path, exist_ok=True)
    torch.save({
        'config': cfg,
        'epoch': epoch,
        'model_state_dict': model.state_dict(),
        'optimizer_state_dict': optimizer.state_dict(),
        'scheduler_state_dict': None if scheduler is None else scheduler.state_dict(),
        'anchors': model.anchors,
        'val_anet_metrics': anet_metrics,
        'best_metric': best_metric,
    }, os.path.join(cfg.log_path, 'best_prop_model.pt'))


def train_av_loop(cfg, model, optimizer, loader, epoch, TBoard):
    model.train()
    total_loss = 0
    acc_A, acc_V = {}, {}
    for batch in loader:
        optimizer.zero_grad()
        masks = make_masks(batch['feature_stacks'], None, cfg.modality, loader.dataset.pad_idx)
        _, loss, losses_A, losses_V = model(batch['feature_stacks'], batch['targets'], masks)
        acc_A = add_dict_to_another_dict(losses_A, acc_A)
        acc_V = add_dict_to_another_dict(losses_V, acc_V)
        loss.backward()
        if cfg.grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_clip)
        optimizer.step()
        total_loss += loss.item()
    n = len(loader)
    total_loss /= n
    acc_A = {k: float(v) / n for k, v in acc_A.items()}
    acc_V = {k: float(v) / n for k, v in acc_V.items()}
    if TBoard is not None:
        TBoard.add_scalar('debug/loss_epoch', total_loss, epoch)
        TBoard.add_scalar('debug/lr', get_lr(optimizer), epoch)
        for name, value in acc_A.items():
            TBoard.add_scalar(f'debug/train_{name}_A', value, epoch)
        for name, value in acc_V.items():
            TBoard.add_scalar(f'debug/train_{name}_V', value, epoch)
    else:
        print(f'Train Loss @ {epoch} epoch: {total_loss}')
    return total_loss, acc_A, acc_V


def validation_loop(cfg, model, optimizer, scheduler, loader, epoch, best_metric, TBoard):
    model.eval()
    anet_predictions = AnetPredictions(cfg, loader.dataset.phase, epoch)
    for batch in loader:
        masks = make_masks(batch['feature_stacks'], None, cfg.modality, loader.dataset.pad_idx)
        with torch.no_grad():
            predictions, _, _, _ = model(batch['feature_stacks'], batch['targets'], masks)
            anet_predictions.add_new_predictions(predictions, batch)
    # val_1 and val_2 share their proposals and both files are references of the evaluation: written once (val_1)
    anet_predictions.write_anet_predictions_to_json()
    anet_metrics = anet_predictions.evaluate_predictions()
    avg_precision = anet_metrics['Average across tIoUs']['Precision']
    avg_recall = anet_metrics['Average across tIoUs']['Recall']
    avg_f1 = calculate_f1(avg_recall, avg_precision)
    if TBoard is not None:
        for tIoU in cfg.tIoUs:
            precision, recall = anet_metrics[tIoU]['Precision'], anet_metrics[tIoU]['Recall']
            TBoard.add_scalar(f'densevid_eval_k/precision_{tIoU}', precision, epoch)
            TBoard.add_scalar(f'densevid_eval_k/recall_{tIoU}', recall, epoch)
            TBoard.add_scalar(f'densevid_eval_k/F1_{tIoU}', calculate_f1(recall, precision), epoch)
        TBoard.add_scalar('metrics/avg_precision_at_k', avg_precision, epoch)
        TBoard.add_scalar('metrics/avg_recall_at_k', avg_recall, epoch)
        TBoard.add_scalar('metrics/avg_F1_at_k', avg_f1, epoch)
        # AR@AN and its area (cfg.proposal_evaluator_options = {..., "proposal_recall": True}; bmhrl_amd/evaluate.py)
        for key, tag in (('AUC', 'metrics/AUC'), ('AR@AN', 'metrics/AR_at_AN')):
            if key in anet_metrics['Average across tIoUs']:
                TBoard.add_scalar(tag, anet_metrics['Average across tIoUs'][key], epoch)
    if scheduler is not None:
        scheduler.step(avg_f1)
    if avg_f1 > best_metric and TBoard is not None:
        best_metric = avg_f1
        save_model(cfg, epoch, model, optimizer, scheduler, anet_metrics, best_metric)
        print(f'Saved model @ {epoch} epoch. Best metric: {best_metric:.5f}')
    return best_metric
