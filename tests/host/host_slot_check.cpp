/*
 * host_slot_check.cpp -- csrc/rdsp_slot.h, the double-buffering of rdsp_chain_t's per-group tables, as a program of its own:
 * plain C++, nothing of HIP, built with -fsanitize=address,undefined.
 *
 * Walks every sequence of fill (F) and switch_over (S) of up to MAX_LEN steps from a fresh slot, and again from a slot
 * that was reset behind "FS", "FSF" and "F" (live 1; live 1 with a pending half; a pending half alone).  At every step:
 *   - a fill never targets the half `live` names;
 *   - two fills with no switch between them target the same half;
 *   - images alternate: the image of a fill is the one of two fills earlier, never the previous one's;
 *   - after a switch, `live` is the last fill's target and nothing is pending; without a pending half it changes nothing;
 *   - (image, target, live) are those of the mask staging as rdsp_chain_groups.hip wrote it out before the slot existed,
 *     transcribed below (Before).
 * Prints "host_slot_check OK" and the number of steps checked.
 */
#include <stdio.h>

#include "rdsp_slot.h"

static const int MAX_LEN = 12;

/* chain_group_stage and chain_groups_commit as they were: si = next; target = staged >= 0 ? staged : 1 - applied;
 * last = si; next = si ^ 1; staged = target -- and: if (staged >= 0) { applied = staged; staged = -1; } */
struct Before {
  int applied = 0, staged = -1, next = 0, last = 0;
  rdsp_slot::Fill stage() {
    const int si = next;
    const int target = (staged >= 0) ? staged : (1 - applied);
    last = si;
    next = si ^ 1;
    staged = target;
    return {si, target};
  }
  void commit() {
    if (staged >= 0) {
      applied = staged;
      staged = -1;
    }
  }
};

struct Walk {
  rdsp_slot::Slot s;
  Before b;
  int fills = 0;            /* so far */
  int image1 = -1;          /* the image of the last fill, of the one before it */
  int image2 = -1;
  int target_since = -1;    /* the target of the fills since the last switch; -1: none */
};

static long g_steps = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) { printf("FAIL %s (line %d) after %s\n", #cond, __LINE__, path); return false; } \
  } while (0)

static bool same(const rdsp_slot::Slot &s, const Before &b) {
  return s.live == b.applied && s.pending == b.staged && s.next_image == b.next && s.last_image == b.last;
}

static bool step(Walk &w, char op, const char *path) {
  g_steps++;
  if (op == 'F') {
    const int live = w.s.live;
    const rdsp_slot::Fill f = w.s.fill(), want = w.b.stage();
    CHECK(f.image == want.image && f.target == want.target);
    CHECK(f.image == 0 || f.image == 1);
    CHECK(f.target == 0 || f.target == 1);
    CHECK(f.target != live && w.s.live == live);
    CHECK(w.target_since < 0 || f.target == w.target_since);
    CHECK(w.image1 < 0 || f.image != w.image1);
    CHECK(w.image2 < 0 || f.image == w.image2);
    CHECK(w.s.pending == f.target && w.s.last_image == f.image && w.s.next_image == (f.image ^ 1));
    w.image2 = w.image1;
    w.image1 = f.image;
    w.target_since = f.target;
    w.fills++;
  } else {
    const rdsp_slot::Slot was = w.s;
    w.s.switch_over();
    w.b.commit();
    if (w.target_since >= 0) {
      CHECK(was.pending == w.target_since);
      CHECK(w.s.live == w.target_since && w.s.pending < 0);
    } else {
      CHECK(was.pending < 0);
      CHECK(w.s.live == was.live && w.s.pending == was.pending);
    }
    CHECK(w.s.next_image == was.next_image && w.s.last_image == was.last_image);
    w.target_since = -1;
  }
  CHECK(same(w.s, w.b));
  return true;
}

static bool walk(const Walk &w, char *path, int len) {
  if (len == MAX_LEN) return true;
  for (const char *op = "FS"; *op; op++) {
    Walk n = w;
    path[len] = *op;
    path[len + 1] = 0;
    if (!step(n, *op, path) || !walk(n, path, len + 1)) return false;
  }
  return true;
}

int main() {
  char path[MAX_LEN + 8];
  Walk w;
  path[0] = 0;
  if (!walk(w, path, 0)) return 1;
  /* reset: live and pending as a fresh slot has them, whatever they were; the images go on alternating, which the walk
   * behind it checks (image1 / image2 are kept) */
  for (int pre = 0; pre < 3; pre++) { /* behind F S (live 1), behind F S F (live 1, pending 0), behind F (pending 1) */
    Walk r;
    const char *ops = pre == 0 ? "FS" : pre == 1 ? "FSF" : "F";
    for (const char *op = ops; *op; op++)
      if (!step(r, *op, ops)) return 1;
    r.s.reset();
    if (r.s.live != 0 || r.s.pending != -1) { printf("FAIL reset behind %s\n", ops); return 1; }
    r.b.applied = 0; /* chain_groups_resize as it was: applied = 0, staged = -1, the image indices kept */
    r.b.staged = -1;
    r.target_since = -1;
    path[0] = 0;
    if (!walk(r, path, 0)) return 1;
  }
  printf("host_slot_check OK %ld steps\n", g_steps);
  return 0;
}
