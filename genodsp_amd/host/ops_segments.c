/* ops_segments.c -- segments (device shim).  Not an operator of the reference: the table every peak caller ends in --
 * one line per region of the signal above a threshold, with its count, sum (area), mean, min, max (height) and the
 * position of the maximum (summit).  Regions can be joined across short gaps, and dropped when they are short or never
 * reach a second, higher threshold (hysteresis calling).  The signal is not modified; the variables segments, covered
 * and longest are set.
 *
 * A genome-wide operator like statsover: the driver brings stretches back to whole chromosomes first.  Each device in
 * use gets one gdsp_segments_batch (include/genodsp_hip.h) over its chromosomes in the order of the chromosomes file:
 * the signal is read on the device, the regions and their exact figures arrive here a bounded number at a time, and
 * their lines are written as they arrive.  The table follows the chromosomes file (the order of the final report),
 * positions ascending; a chromosome whose turn has not come yet -- it lives on a device that is served before that of
 * an earlier chromosome -- waits as text (a single device never waits).
 *
 * keepsegments (ops_keepsegments.c) selects its segments by the same options and writes them back into the signal: the
 * options' parser (segments_opts_*) and the pass (segments_run) are here for both.
 *
 * The driver finds both operators through opgroup_segments, at the end of ops_keepsegments.c (host_services.h); every call
 * into the device library for them stays in this file. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_segments)

typedef struct dspop_segments
	{
	dspop   common;
	segments_opts o;                                               /* (shared with keepsegments: host_services.h) */
	int     quiet;
	} dspop_segments;

OP_SHORT (op_segments, "print the regions above a threshold with their count, sum, mean, min, max and summit (not in genodsp)")

void op_segments_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint one line per region of consecutive bases above a threshold: chromosome, start, end,\n", indent);
	fprintf (f, "%sthen the count, sum, mean, min and max of the signal inside the region and the position of\n", indent);
	fprintf (f, "%sthe (first) maximum; sum and mean are exact and rounded once. Regions can be joined across\n", indent);
	fprintf (f, "%sshort gaps (whose bases are not counted) and dropped when they are short or low. Sets the\n", indent);
	fprintf (f, "%svariables segments, covered and longest. The signal is not modified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [<threshold>] [options]\n", indent, name);
	fprintf (f, "%s  <threshold>              numeric threshold (default 0.0)\n", indent);
	fprintf (f, "%s  --threshold=<variable>   (T=) threshold from a named variable, e.g. percentile99\n", indent);
	fprintf (f, "%s  --ties:below|above       whether values equal to the threshold count as below (default) or above\n", indent);
	fprintf (f, "%s  --mergegap=<bases>       join regions no more than this many bases apart (default 0)\n", indent);
	fprintf (f, "%s  --minlength=<bases>      drop regions shorter than this, after joining (default 1)\n", indent);
	fprintf (f, "%s  --minheight=<value|variable>  drop regions whose maximum is below this\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the positions printed\n", indent);
	fprintf (f, "%s  --quiet                  print no table (the variables are still set)\n", indent);
	}

static u32 bases_arg (char* name, char* arg, char* argVal, const char* what)
	{
	u32 v;
	if (*skip_whitespace (argVal) == '-') chastise ("[%s] %s can't be negative (\"%s\")\n", name, what, arg);
	if (!try_string_to_u32 (argVal, &v)) chastise ("[%s] %s must be a number of bases (\"%s\")\n", name, what, arg);
	return v;
	}

void segments_opts_init (segments_opts* o)
	{
	memset (o, 0, sizeof(*o));
	o->minLength = 1;
	o->precision = -1;
	o->originOne = (int) get_named_global ("originOne", false);
	}

/* the threshold as a variable's name and the side of the ties (distance, ops_distance.c, takes these and no more);
 * true: `arg` was one of them */
int segments_threshold_take (segments_opts* o, char* name, char* arg)
	{
	char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
	if (is_opt3 (arg, "threshold", "T"))                 /* a variable NAME only, as binarize */
		{
		if (o->haveThreshold) { fprintf (stderr, "[%s] threshold specified more than once (at \"%s\")\n", name, arg);  exit (EXIT_FAILURE); }
		o->thresholdVarName = copy_string (argVal);
		o->haveThreshold = true;
		return true;
		}
	if ((strcmp (arg, "--ties:below") == 0) || (strcmp (arg, "--ties=below") == 0)) { o->tiesAbove = false;  return true; }
	if ((strcmp (arg, "--ties:above") == 0) || (strcmp (arg, "--ties=above") == 0)) { o->tiesAbove = true;   return true; }
	return false;
	}

/* the options that select the segments and shape their table; true: `arg` was one of them */
int segments_opts_take (segments_opts* o, char* name, char* arg)
	{
	char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
	if (segments_threshold_take (o, name, arg)) return true;
	if (strcmp_prefix (arg, "--mergegap=") == 0)  { o->mergeGap  = bases_arg (name, arg, argVal, "--mergegap");   return true; }
	if (strcmp_prefix (arg, "--minlength=") == 0) { o->minLength = bases_arg (name, arg, argVal, "--minlength");  return true; }
	if (strcmp_prefix (arg, "--minheight=") == 0)
		{
		if (o->minHeightVarName != NULL) { free (o->minHeightVarName);  o->minHeightVarName = NULL; }
		value_or_variable (argVal, &o->minHeight, &o->minHeightVarName);
		o->haveMinHeight = true;
		return true;
		}
	if (strcmp_prefix (arg, "--output=") == 0)
		{ if (o->outFilename != NULL) free (o->outFilename);  o->outFilename = copy_string (argVal);  return true; }
	if (strcmp_prefix (arg, "--precision=") == 0)
		{
		o->precision = string_to_int (argVal);
		if (o->precision < 0) chastise ("[%s] precision can't be negative (\"%s\")\n", name, arg);
		return true;
		}
	return origin_opt_take (arg, &o->originOne);
	}

/* what is left when the operator's own options have had their turn: --debug, an option nobody knows, the threshold */
void segments_opts_take_other (segments_opts* o, char* name, char* arg)
	{
	if (strcmp (arg, "--debug") == 0) return;
	if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
	if (!o->haveThreshold) { o->threshold = string_to_valtype (arg);  o->haveThreshold = true;  return; }
	valtype again;
	if (try_string_to_valtype (arg, &again))
		{ fprintf (stderr, "[%s] threshold specified more than once (at \"%s\")\n", name, arg);  exit (EXIT_FAILURE); }
	chastise ("[%s] Can't understand \"%s\"\n", name, arg);
	}

void segments_opts_free (segments_opts* o)
	{
	if (o->thresholdVarName != NULL) free (o->thresholdVarName);
	if (o->minHeightVarName != NULL) free (o->minHeightVarName);
	if (o->outFilename      != NULL) free (o->outFilename);
	}

dspop* op_segments_parse (char* name, int argc, char** argv)
	{
	dspop_segments* op = (dspop_segments*) new_op (name, sizeof(dspop_segments), true);
	segments_opts_init (&op->o);
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		if (segments_opts_take (&op->o, name, arg)) continue;
		if ((strcmp (arg, "--quiet") == 0) || (strcmp (arg, "--silent") == 0)) { op->quiet = true;  continue; }
		segments_opts_take_other (&op->o, name, arg);
		}
	return (dspop*) op;
	}

void op_segments_free (dspop* _op)
	{
	dspop_segments* op = (dspop_segments*) _op;
	segments_opts_free (&op->o);
	free (op);
	}

/* ------------------------------------------------------------------------------------------- the table ---- */
/* a chromosome of the table, in the order of the chromosomes file */
typedef struct chromtext { spec* s;  int done;  char* text;  size_t len, cap; } chromtext;

typedef struct tablestate
	{
	const segments_opts* op;  const char* name;
	FILE*      out;
	chromtext* chroms;  int numChroms, next;                  /* chroms[next] is the one whose lines go straight out */
	int*       mine;    int numMine, upTo;                    /* this device's vectors as indices into chroms; those before upTo are complete */
	char*      text;    size_t textCap;
	u64        kept, covered, longest;
	} tablestate;

/* every chromosome whose turn has come and that is complete leaves; so does what the next one has waiting */
static void advance (tablestate* t)
	{
	while (t->next < t->numChroms)
		{
		chromtext* c = &t->chroms[t->next];
		if (c->len != 0) { fwrite (c->text, 1, c->len, t->out);  c->len = 0; }
		if (c->text != NULL) { free (c->text);  c->text = NULL;  c->cap = 0; }
		if (!c->done) break;
		t->next++;
		}
	}

/* this device's vectors before `vec` have given all their segments */
static void complete_before (tablestate* t, int vec)
	{
	if (vec <= t->upTo) return;
	for ( ; t->upTo<vec ; t->upTo++) t->chroms[t->mine[t->upTo]].done = true;
	advance (t);
	}

static int take_segments (void* ctx, const gdsp_segment* segs, uint32_t count)
	{
	tablestate* t = (tablestate*) ctx;
	const segments_opts* op = t->op;
	const char* name = t->name;
	const u32   o = op->originOne? 1 : 0;
	size_t len = 0;
	int    held = -1;                                         /* the chromosome the lines in t->text belong to */
	for (uint32_t k=0 ; k<=count ; k++)
		{
		const int ci = (k < count)? t->mine[segs[k].vec] : -1;
		if ((len != 0) && ((ci != held) || (len + 2400 > t->textCap)))
			{
			chromtext* c = &t->chroms[held];
			if (held == t->next) fwrite (t->text, 1, len, t->out);
			else
				{
				if (c->len + len > c->cap)
					{
					c->cap  = 2 * (c->len + len) + 4096;
					c->text = (char*) must_alloc (realloc (c->text, c->cap), name);
					}
				memcpy (c->text + c->len, t->text, len);  c->len += len;
				}
			len = 0;
			}
		if (k == count) break;
		complete_before (t, (int) segs[k].vec);
		held = ci;
		const gdsp_segment* g = &segs[k];
		spec* s = t->chroms[ci].s;
		t->kept++;  t->covered += g->end - g->start;
		if (g->end - g->start > t->longest) t->longest = g->end - g->start;
		if (t->out == NULL) continue;                         /* (no table: the variables are still set) */
		const size_t chromLen = strlen (s->chrom);
		if (chromLen + 2400 > t->textCap)
			{
			t->textCap = (1u << 20) + chromLen + 2400;
			t->text = (char*) must_alloc (realloc (t->text, t->textCap), name);
			}
		char* p = t->text + len;
		memcpy (p, s->chrom, chromLen);  p += chromLen;  *(p++) = '\t';
		p = put_unsigned (p, (unsigned long long) s->start + g->start + o);  *(p++) = '\t';
		p = put_unsigned (p, (unsigned long long) s->start + g->end);
		p = put_interval_figures (p, &g->stat, s->start, op->originOne, op->precision);
		len = (size_t) (p - t->text);
		}
	return 0;
	}

/* the pass of `segments`, and of keepsegments when `paint` is given: then every chromosome's partner is painted from the
 * kept segments and becomes the signal */
void segments_run (dspop* _op, segments_opts* op, int wantTable, const segments_paint* paint)
	{
	char* name = _op->name;
	resolve_variable (_op, &op->thresholdVarName, &op->threshold, "threshold");
	if (op->haveMinHeight) resolve_variable (_op, &op->minHeightVarName, &op->minHeight, "minimum height");
	if (op->threshold != op->threshold) { fprintf (stderr, "[%s] the threshold is not a number\n", name);  exit (EXIT_FAILURE); }
	if (op->haveMinHeight && (op->minHeight != op->minHeight)) { fprintf (stderr, "[%s] the minimum height is not a number\n", name);  exit (EXIT_FAILURE); }

	tablestate t;
	memset (&t, 0, sizeof(t));
	t.op = op;  t.name = name;
	for (spec* s=chromsOfInterest ; s!=NULL ; s=s->next) t.numChroms++;
	t.chroms = (chromtext*) must_alloc (calloc (t.numChroms + 1, sizeof(chromtext)), name);
	t.mine   = (int*) must_alloc (calloc (t.numChroms + 1, sizeof(int)), name);
	gdsp_batch_item* items = (gdsp_batch_item*) must_alloc (calloc (t.numChroms + 1, sizeof(gdsp_batch_item)), name);
		{
		int ci = 0;
		for (spec* s=chromsOfInterest ; s!=NULL ; s=s->next) t.chroms[ci++].s = s;
		}
	t.out = wantTable? open_table (name, op->outFilename) : NULL;

	sync_all_devices ();
	for (int d=0 ; d<device_count_in_use () ; d++)            /* one launch sequence per device, its chromosomes in file order */
		{
		t.numMine = 0;  t.upTo = 0;
		for (int ci=0 ; ci<t.numChroms ; ci++)
			{
			spec* s = t.chroms[ci].s;
			if (device_index_of (s) != d) continue;
			if (trackOperations) fprintf (stderr, "%s(%s)\n", name, s->chrom);
			items[t.numMine].d_in = s->valVector;  items[t.numMine].d_out = (paint != NULL)? partner_of (s) : NULL;  items[t.numMine].n = s->length;
			t.mine[t.numMine++] = ci;
			}
		if (t.numMine == 0) continue;
		select_device_of (t.chroms[t.mine[0]].s);
		if (paint == NULL)
			check_gdsp (gdsp_segments_batch (items, t.numMine, op->threshold, op->tiesAbove, op->mergeGap, op->minLength,
			                                 op->haveMinHeight, op->minHeight, take_segments, &t, op_stream ()), name);
		else
			{
			check_gdsp (gdsp_keep_segments_batch (items, t.numMine, op->threshold, op->tiesAbove, op->mergeGap, op->minLength,
			                                      op->haveMinHeight, op->minHeight, paint->mode, paint->one, paint->zero,
			                                      take_segments, &t, op_stream ()), name);
			for (int k=0 ; k<t.numMine ; k++) flip_vector (t.chroms[t.mine[k]].s->chrom);     /* what was painted is the signal now */
			}
		if (t.out != NULL) complete_before (&t, t.numMine);
		}
	select_device_of (chromsSorted[0]);
	if (t.out != NULL) close_table (t.out);

	set_named_global ("segments", (valtype) t.kept);
	set_named_global ("covered",  (valtype) t.covered);
	set_named_global ("longest",  (valtype) t.longest);
	for (int ci=0 ; ci<t.numChroms ; ci++) free (t.chroms[ci].text);
	free (t.chroms);  free (t.mine);  free (items);  free (t.text);
	}

void op_segments_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_segments* op = (dspop_segments*) _op;
	segments_run (_op, &op->o, !op->quiet, NULL);
	}
