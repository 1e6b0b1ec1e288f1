// The fields of a column item and their refusals, for k_prog_columns and k_prog_columns_weighted.  Included as text (DESIGN.md
// §3a); the kernel provides its parameters (max_kind among them: the highest kind it accepts, 1 or 2), the fields buf, off, R, W, kind, coff (long long, zero) behind which it declares its
// own, PG_ITEM_STRIDE, the words of an item, PG_ITEM_READ_MORE, statements that read its own fields of the item I, and PG_ITEM_ALSO_BAD, its own further refusals: the end of the || chain below, so clauses joined
// by || and no brackets around them (false: none).  Defines it, tile and st (MPRG_PG_OK, or why the item is refused) and
// fills in the fields.
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long it = wk[0], tile = wk[1];
  int st = MPRG_PG_OK;
  if (it < 0 || it >= n_items) st = MPRG_PG_BAD_ITEM;
  else {
    const int64_t *I = items + PG_ITEM_STRIDE * it;
    buf = I[0]; off = I[1]; R = I[2]; W = I[3]; kind = I[4]; coff = I[5];
    PG_ITEM_READ_MORE
    if (!pg_text_ok(bufs, n_bufs, buf, off, R, W) || tile < 0 || tile * 256 >= W || kind < 0 || kind > max_kind || PG_ITEM_ALSO_BAD)
      st = MPRG_PG_BAD_ITEM;
    else if (coff < 0 || coff > cols_words || (kind == 0 ? 6 : 7) * W > cols_words - coff) st = MPRG_PG_NO_SPACE;
  }
