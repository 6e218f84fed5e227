/* tools/throttle_ref_host.c -- DEVELOPMENT-MACHINE TOOL of tools/gen_throttle_golden.py.  Drives the reference's own filter_throttle_size
 * or filter_throttle through a script of steps and records cb_filter's answers.  The plugin is compiled where it lies in a fluent-bit
 * source tree into one loadable flb-filter_<name>.so, linked with --wrap=sleep, --wrap=flb_time_get and --wrap=flb_log_print; this host defines the
 * wrappers (it is linked with -rdynamic), loads the plugin with flb_plugin_load_router and links the reference engine library
 * (oracle/_ref/engine).
 *
 *   throttle_ref_host <plugin.so> <throttle_size|throttle> <script> [name=value]...
 *
 * The script: one step a line -- "now T", "tick T", "chunk <hex>".  The plugin's ticker thread runs its OWN loop body, at the script's
 * times and at no others: every trip begins with flb_time_get, and the wrapper, called off the main thread, waits there for a `tick`
 * step (sem_wait: a cancellation point, filter_throttle ends its ticker by pthread_cancel) and answers that step's time; sleep returns
 * at once.  The host waits for the ticker's arrival at the gate before the first step and after every tick, so a trip is over when
 * its step is.  flb_time_get on the main thread (size_window_create) answers the last `now`; `now` lines in front of the first other
 * step are applied before cb_init.  One JSON line on stdout per chunk step: {"ret": <cb_filter's answer>, "out": "<hex>"}; in front
 * of them {"init": true|false}.  The process leaves by _exit: the gated ticker is never joined.
 *   --repeat-ns n (behind the script): the last chunk step is called n times more and the fastest call's time is printed as
 *   {"filter_ns": t} (tools/perf_throttle_size.py --cpu-reference). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include <unistd.h>
#include <pthread.h>
#include <semaphore.h>
#include <fluent-bit.h>
#include <fluent-bit/flb_info.h>
#include <fluent-bit/flb_config.h>
#include <fluent-bit/flb_plugin.h>
#include <fluent-bit/flb_filter.h>
#include <fluent-bit/flb_input.h>
#include <fluent-bit/flb_processor.h>
#include <fluent-bit/flb_time.h>

static pthread_t main_thread;
static sem_t arrived, go;
static volatile long now_time = 0, tick_time = 0;

int __wrap_flb_time_get(struct flb_time *tm)
{
    if (pthread_equal(pthread_self(), main_thread)) {
        tm->tm.tv_sec = now_time;
        tm->tm.tv_nsec = 0;
        return 0;
    }
    sem_post(&arrived);
    while (sem_wait(&go) != 0) { }
    tm->tm.tv_sec = tick_time;
    tm->tm.tv_nsec = 0;
    return 0;
}

/* The plugins' log lines are dropped (the .so is linked with --wrap=flb_log_print as well): when filter_throttle_size deletes a stale
 * window it frees it and then formats the freed window's name into an info line (throttle_size.c:133-145), which ends a process
 * whose allocator has reused the bytes.  Without the line the deletion itself is what the reference does. */
void __wrap_flb_log_print(int type, const char *file, int line, const char *fmt, ...)
{
    (void) type; (void) file; (void) line; (void) fmt;
}

unsigned int __wrap_sleep(unsigned int seconds)
{
    (void) seconds;
    return 0;
}

static size_t unhex(const char *s, unsigned char *out)
{
    size_t n = 0;
    unsigned int v;
    while (s[0] && s[1] && sscanf(s, "%2x", &v) == 1) { out[n++] = (unsigned char) v; s += 2; }
    return n;
}

int main(int argc, char **argv)
{
    struct flb_config *config;
    struct flb_processor *proc;
    struct flb_processor_unit *pu;
    struct flb_filter_instance *f_ins;
    FILE *fs;
    char *line = NULL;
    size_t cap = 0, i;
    ssize_t got;
    int k, started = 0, repeat = 0;
    unsigned char *buf = NULL, *last = NULL;
    size_t last_len = 0;

    if (argc < 4) { fprintf(stderr, "usage: throttle_ref_host <plugin.so> <name> <script> [--repeat-ns n] [name=value]...\n"); return 2; }
    main_thread = pthread_self();
    sem_init(&arrived, 0, 0);
    sem_init(&go, 0, 0);
    fs = fopen(argv[3], "r");
    if (!fs) { perror(argv[3]); return 2; }
    k = 4;
    if (argc > 5 && !strcmp(argv[4], "--repeat-ns")) { repeat = atoi(argv[5]); k = 6; }
    flb_init_env();
    config = flb_config_init();
    if (!config) return 1;
    if (flb_plugin_load_router(argv[1], config) != 0) { fprintf(stderr, "flb_plugin_load_router(%s) failed\n", argv[1]); return 3; }
    proc = flb_processor_create(config, "throttle_ref_host", NULL, 0);
    if (!proc) return 1;
    pu = flb_processor_unit_create(proc, FLB_PROCESSOR_LOGS, argv[2]);
    if (!pu) { fprintf(stderr, "flb_processor_unit_create(%s) failed\n", argv[2]); return 3; }
    for (; k < argc; k++) {
        char *kv = strdup(argv[k]), *eq = strchr(kv, '=');
        if (!eq) { fprintf(stderr, "bad property %s\n", argv[k]); return 2; }
        *eq = 0;
        if (flb_processor_unit_set_property_str(pu, kv, eq + 1) != 0) { printf("{\"init\": false, \"property\": \"%s\"}\n", kv); fflush(stdout); _exit(0); }
        free(kv);
    }
    f_ins = NULL;
    while ((got = getline(&line, &cap, fs)) >= 0) {
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) line[--got] = 0;
        if (!strncmp(line, "now ", 4)) { now_time = atol(line + 4); if (!started) continue; }
        if (!started) {
            if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); fflush(stdout); _exit(0); }
            f_ins = pu->ctx;
            f_ins->log_level = FLB_LOG_WARN;
            while (sem_wait(&arrived) != 0) { }                 /* the ticker stands at the gate of its first trip */
            printf("{\"init\": true}\n");
            started = 1;
        }
        if (!strncmp(line, "now ", 4)) continue;
        if (!strncmp(line, "tick ", 5)) {
            tick_time = atol(line + 5);
            sem_post(&go);
            while (sem_wait(&arrived) != 0) { }                 /* the trip is over: the ticker is back at the gate */
        }
        else if (!strncmp(line, "chunk", 5)) {
            const char *hex = line[5] == ' ' ? line + 6 : line + 5;
            void *out_buf = NULL;
            size_t out_size = 0, n;
            int ret;
            buf = realloc(buf, strlen(hex) / 2 + 1);
            n = unhex(hex, buf);
            ret = f_ins->p->cb_filter(buf, n, "t", 1, &out_buf, &out_size, f_ins, NULL, f_ins->context, config);
            printf("{\"ret\": %d, \"out\": \"", ret);
            if (ret == FLB_FILTER_MODIFIED) for (i = 0; i < out_size; i++) printf("%02x", ((unsigned char *) out_buf)[i]);
            printf("\"}\n");
            if (ret == FLB_FILTER_MODIFIED && out_buf) free(out_buf);
            last = realloc(last, n + 1); memcpy(last, buf, n); last_len = n;
        }
    }
    if (!started) {
        if (flb_processor_init(proc) != 0) { printf("{\"init\": false}\n"); fflush(stdout); _exit(0); }
        printf("{\"init\": true}\n");
        f_ins = pu->ctx;
    }
    if (repeat > 0 && last) {
        long long best = -1;
        int r;
        for (r = 0; r < repeat; r++) {
            struct timespec t0, t1;
            void *out_buf = NULL;
            size_t out_size = 0;
            long long ns;
            int ret;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            ret = f_ins->p->cb_filter(last, last_len, "t", 1, &out_buf, &out_size, f_ins, NULL, f_ins->context, config);
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if (ret == FLB_FILTER_MODIFIED && out_buf) free(out_buf);
            ns = (long long) (t1.tv_sec - t0.tv_sec) * 1000000000LL + (t1.tv_nsec - t0.tv_nsec);
            if (best < 0 || ns < best) best = ns;
        }
        printf("{\"filter_ns\": %lld}\n", best);
    }
    fflush(stdout);
    _exit(0);
}
