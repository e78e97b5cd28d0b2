"""The contract of cc_logits_constrain / cc_token_history_write (include/coldcompress.h) restated in plain Python, independently of
cold_compress_amd/harness/constraints.py: lists of ints in, the banned set out; rows in, rows out.

A row computed at position p has the history s[0 .. p] (prompt, then decode inputs, by absolute position) and predicts the token at
p + 1.  A banned element becomes -inf, every other keeps its bits: there is no arithmetic, hence no tolerance.  (The row families and
the bitwise comparison are tests/penalty_twin.py's.)"""

SLICE = 1024  # (CC_CONSTRAIN_SLICE: candidate starts per workgroup of the ban pass)


def ngram_bans(s, n, first=0):
    """HF's NoRepeatNGramLogitsProcessor on the list s, counting only n-grams that start at `first` or later: every n-gram of s is
    filed under its first n - 1 tokens; what is filed under the last n - 1 tokens of s is banned."""
    if n <= 0 or len(s) + 1 < n:
        return set()
    filed = {}
    for i in range(max(first, 0), len(s) - n + 1):
        gram = tuple(s[i:i + n])
        filed.setdefault(gram[:-1], set()).add(gram[-1])
    key = tuple(s[len(s) - (n - 1):]) if n > 1 else ()
    return set(filed.get(key, ()))


def min_length_bans(s, gen_start, m, terminators):
    return set(terminators) if len(s) - gen_start < m else set()


def bad_word_bans(s, bad_words):
    """PER SEQUENCE: w bans its last token when the tokens in front of it are the end of s (a one-token w: always)."""
    out = set()
    for w in bad_words:
        head, last = list(w[:-1]), w[-1]
        if not head or (len(head) <= len(s) and s[len(s) - len(head):] == head):
            out.add(last)
    return out


def banned(s, gen_start=0, n=0, scope="all", m=0, terminators=(), bad_words=()):
    """The banned ids of the row whose history is the list s (its position is len(s) - 1)."""
    assert scope in ("all", "generated")
    return (ngram_bans(s, n, gen_start if scope == "generated" else 0) | min_length_bans(s, gen_start, m, terminators)
            | bad_word_bans(s, bad_words))


def twin(rows, hist, tokens, pos0, gen_start, **rules):
    """rows [T, V] (CPU tensor), hist: list of ints (len(hist) = cap), tokens: T ints or None, pos0: the first row's position.
    -> (out [T, V], hist' as a list): row t sits at pos0 + t; its history is hist in front of pos0 (everywhere with tokens None) and
    the block's own tokens from pos0 on; rows at positions outside [0, cap) are copied and store nothing."""
    T, V = rows.shape
    cap = len(hist)
    out = rows.clone()
    new_hist = list(hist)
    for t in range(T):
        p = pos0 + t
        if p < 0 or p >= cap:
            continue
        s = [hist[j] if (tokens is None or j < pos0) else tokens[j - pos0] for j in range(p + 1)]
        for w in banned(s, gen_start, **rules):
            if 0 <= w < V:
                out[t, w] = -float("inf")
        if tokens is not None:
            new_hist[p] = tokens[t]
    return out, new_hist
